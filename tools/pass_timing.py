"""Time per time step of the forward run and of the derivative passes, one family of passes per call.

    python tools/pass_timing.py --family FAMILY [--config C] [--nsrc N] [--nfreq F] [--ntimes T] [--repeats R]
                                [--only PASS ...] [--profile PASS] [--package DIR]

    family          passes                                                          default configuration
    adjoint         forward adjoint                                                 C3, 2 channels
    basis_adjoint   forward fluxes beam_coefs both                                  C5, 4 channels  (--small: HERA-37, K = 3)
    position        forward position                                                C3, 8 channels  (--array)
    source          forward fluxes sources joint                                    C3, 8 channels
    tangent         forward position source tangent_baselines tangent_directions
                    tangent_both                                                    C3, 8 channels  (--array)
    basis_tangent   forward tangent_1 tangent_n beam_coefs                          C5, 8 channels  (--ndir)
    basis_position  forward adjoint tangent                                         C5, 8 channels
    basis_source    forward fluxes tangent_ants source_adjoint source_tangent
                    joint                                                           C5, 8 channels  (--precision)
    objective       forward separate separate_torch fused fused_device              C3, 8 channels  (--wrt, --lattice,
                                                                                    --gains; --config C5: through K = 4)
    gauss_newton    forward composed fused fused_device                             C3, 8 channels  (--case, --gains,
                                                                                    --d-gains, --jones, --d-jones;
                                                                                    beam_coefs: --config C5)
    gain_solve      forward solve solve_with_forward gauss_newton_products          C3, 8 channels
    jones_solve     forward solve solve_with_forward jones_chi2_steps               C3, 8 channels
    redundant_solve solve gain_solve both                                           C3, 8 channels
    firstcal        firstcal solve                                                  C3, 8 channels
    abscal          abscal model_groups model_all gain_solve fix                    C3, 8 channels

Prints one JSON line: ms per time step of each pass (wall clock of a whole call on a warm handle, divided by the time
steps; the median of --repeats calls, with the values or their range) and the family's ratios, under the keys the family
has always printed.  --only PASS (repeatable) times those passes alone: ``--only forward`` is what runs on a checkout from
before the family's passes.  --profile PASS: one call of that pass on a cold handle and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/pass_timing.py --family source --profile sources).  --package: the
checkout whose fftvis_amd is measured (an earlier commit's, built in place; default: this one).  --array surveyed
(position, tangent): seeded N(0, 2 cm) errors in x, y and 3 cm in z on the ideal array.  --lattice (adjoint): the
reference's default call on a griddable array (force_use_type3=False: the forward is the type-1 transform);
--adjoint-path (adjoint): the adjoint's transform there.  objective: one iteration of a fit, chi2 = sum w |V - d|^2 and its
gradients -- ``separate`` is simulate_vis, then numpy, then the public adjoint on the host result (runs on a checkout from
before the fused call, as ``forward`` does: --package DIR --only forward --only separate), ``separate_torch`` the torch
operation, a torch loss and .backward() (fluxes only), ``fused`` simulate_vis_chi2 on host data and ``fused_device`` on
resident tensors; --wrt NAMES (comma-separated, default fluxes) selects the gradients, --lattice the type-1 forward; the
line also holds the bytes each variant moves across PCIe per call, from the shapes; --gains puts per-antenna gains into
the data model (``gains`` may then be one of --wrt's names): ``fused`` and ``fused_device`` call ``simulate_vis_gain_chi2`` (resident gains
for the latter), ``separate`` becomes the forward to the host, the gain product and the loss in torch, .backward() and the
public adjoints on the host result, and ``--profile gain_kernels`` runs the kernels of fv_gain_residual_chi2 (k_gain_gradient,
k_residual_rows<T, true>) and of fv_residual_chi2 (k_residual_rows<T, false>) alone on the
block's shape, six times each, alternating; --jones puts one 2 x 2 matrix per antenna there instead (``jones`` among
--wrt's names): ``fused`` and ``fused_device`` call ``simulate_vis_jones_chi2``, there is no ``separate``, and ``--profile
jones_kernels`` runs the kernels of fv_jones_residual_chi2, fv_gain_residual_chi2 and fv_residual_chi2 alone the same way.
gauss_newton: one product
2 J^T W J p of a conjugate-gradient solve -- ``composed`` is the public tangent to the host, numpy's 2 w U and the public adjoint
on the host result (runs on a checkout from before the fused call: --package DIR --only forward --only composed), ``fused``
simulate_vis_gauss_newton on host weights and ``fused_device`` on resident weights; --case fluxes | ants | fluxes_radec |
beam_coefs | gains names the direction and the products; ``--profile kernels`` runs k_weight_rows<T, 1, false> and
k_residual_rows<T, false> alone on the block's shape, six times each, alternating.  --gains puts per-antenna gains into the data model and --d-gains adds a gain
direction and the gain block of the product (``--case gains``: that direction alone): ``fused`` and ``fused_device`` call
``simulate_vis_gain_gauss_newton``, ``composed`` becomes the tangent and, with --d-gains, the forward to the host, the gain
product, its tangent, conj(m) 2 w U' and the antennas' sums in torch on the device and the public adjoint on the host
result, and ``--profile gain_kernels`` runs the kernels of fv_gain_weight_rows, fv_weight_rows and fv_gain_residual_chi2 alone
on the block's shape, six times each, alternating.  --jones puts one 2 x 2 matrix per antenna there instead and --d-jones adds
a direction of such matrices and the matrices' block of the product (``--case jones``: that direction alone): ``fused`` and
``fused_device`` call ``simulate_vis_jones_gauss_newton``, ``gain_fused_device`` is ``simulate_vis_gain_gauss_newton`` with the
diagonal of the same matrices and of the same direction in the same job, ``composed`` becomes the tangent and, with
--d-jones, the forward to the host, the 2 x 2 products, 2 w U', the transposed product and the antennas' sums in numpy and the
public adjoint on the host result (on a checkout from before the call: --package DIR --only composed --only
gain_fused_device), and ``--profile jones_kernels`` runs the kernels of fv_jones_weight_rows, fv_gain_weight_rows and
fv_weight_rows alone on the block's shape, six times each, alternating.  gain_solve: the gains-only solve against a fixed model, 50 iterations
per call (every value is the call's wall clock divided by the time steps, as everywhere) -- ``solve`` is
simulate_vis_gain_solve on a resident model with resident data and weights, ``solve_with_forward`` the same from the sky (one
forward, then the iterations), ``gauss_newton_products`` as many gains-only products of simulate_vis_gain_gauss_newton, each
of which reruns the forward (``--profile solve`` for a kernel trace).  jones_solve: the same for the 2 x 2 matrices --
``solve`` and ``solve_with_forward`` call simulate_vis_jones_solve with no sample flagged, ``jones_chi2_steps`` is as many
calls of simulate_vis_jones_chi2 with its gradient, each of which reruns the forward.  redundant_solve: ``solve`` is
redundant_gain_solve on resident data and weights, every baseline of the array in group order, ``gain_solve``
simulate_vis_gain_solve on the same block against the resident model U[group], 50 iterations each and no forward anywhere
(``--only solve --only gain_solve``; ``--profile both`` runs one of each for a kernel trace).  firstcal: ``firstcal`` is
redundant_firstcal on resident data whose gains carry delays of up to 150 ns, channels of 0.5 MHz, 50 iterations of its second
stage, ``solve`` redundant_gain_solve from the firstcal gains, 50 iterations (``--profile firstcal`` for a kernel trace).
abscal: ``abscal`` is redundant_abscal (pad 4, 6 rounds) on resident group visibilities, model and weights, one unit per
channel; ``model_groups`` is simulate_vis on one baseline per group, the model it needs; the other three are the route to
the same end without it: ``model_all`` simulate_vis on every baseline, ``gain_solve`` simulate_vis_gain_solve on that block
against the resident model, 50 iterations, and ``fix`` fix_redundant_degeneracies against its gains (``--profile abscal`` for
a kernel trace).  A flag of another family is an error.
tools/adjoint_timing.sh runs the adjoint family for C2 and C3 and two kernel-trace profiles."""

import argparse
import json
import os
import sys
import time

import numpy as np


def surveyed(ants, seed=2):
    """The array with seeded survey errors: N(0, 2 cm) in x and y, N(0, 3 cm) in z."""
    rng = np.random.default_rng(seed)
    err = rng.normal(size=(len(ants), 3)) * np.array([0.02, 0.02, 0.03])
    return {k: np.asarray(p, float) + err[i] for i, (k, p) in enumerate(ants.items())}


def small_basis_config(fv, nfreq, ntimes):
    """HERA-37 (C2's array), 1e4 sources, three Airy dishes as basis beams, random coefficients, fp64, eps 6e-8."""
    cfg = fv.synth.make_config("C2", nfreq=nfreq, ntimes=ntimes)
    rng = np.random.default_rng(1)
    nant = len(cfg["ants"])
    coefs = 0.05 * (rng.normal(size=(nant, 3, nfreq)) + 1j * rng.normal(size=(nant, 3, nfreq)))
    coefs[:, 0, :] += 1.0
    cfg.update(polarized=True, beam=[fv.AiryBeam(d) for d in (14.0, 13.0, 15.0)], beam_coefs=coefs)
    return cfg


# Every family: (head, calls) from the parsed arguments, the package, the configuration and a seeded generator.  ``head``
# holds the JSON line's leading keys, ``calls`` the passes by name; the gradient G is drawn first, as it always was.

def _g(a, cfg, rng, cast=False):
    nbls = len(cfg["baselines"])
    g = rng.normal(size=(a.nfreq, a.ntimes, 2, 2, nbls) if cfg["polarized"] else (a.nfreq, a.ntimes, nbls)) + 0j
    return g.astype(np.complex64 if cfg["precision"] == 1 else np.complex128) if cast else g


def adjoint(a, fv, cfg, rng):
    if a.lattice:
        cfg["force_use_type3"] = False
    g = _g(a, cfg, rng)
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    if a.adjoint_path != "type3":  # (the default is left out: a checkout from before the keyword takes the same call)
        kw["adjoint_path"] = a.adjoint_path
    head = {"config": a.config, "polarized": bool(cfg["polarized"]), "lattice": bool(a.lattice), "adjoint_path": a.adjoint_path}
    return head, {"forward": lambda: fv.simulate_vis(**cfg), "adjoint": lambda: fv.simulate_vis_adjoint(g, **kw)}


def basis_adjoint(a, fv, cfg, rng):
    g = _g(a, cfg, rng, cast=True)
    calls = {"forward": lambda: fv.simulate_vis(**cfg)}
    for name, wrt in (("fluxes", "fluxes"), ("beam_coefs", "beam_coefs"), ("both", ("fluxes", "beam_coefs"))):
        calls[name] = lambda wrt=wrt: fv.simulate_vis_basis_adjoint(g, **cfg, wrt=wrt)
    return {"config": "small" if a.small else a.config, "nbasis": len(cfg["beam"]), "precision": cfg["precision"]}, calls


def position(a, fv, cfg, rng):
    g = _g(a, cfg, rng)
    return {"array": a.array, "precision": cfg["precision"]}, {
        "forward": lambda: fv.simulate_vis(**cfg),
        "position": lambda: fv.simulate_vis_position_adjoint(g, **cfg, wrt="ants")}


def source(a, fv, cfg, rng):
    g = _g(a, cfg, rng)
    no_flux = {k: v for k, v in cfg.items() if k != "fluxes"}
    return {"precision": cfg["precision"], "polarized": bool(cfg["polarized"])}, {
        "forward": lambda: fv.simulate_vis(**cfg),
        "fluxes": lambda: fv.simulate_vis_adjoint(g, **no_flux, full_stokes=np.ndim(cfg["fluxes"]) == 3),
        "sources": lambda: fv.simulate_vis_source_adjoint(g, **cfg, wrt="radec"),
        "joint": lambda: fv.simulate_vis_sky_adjoint(g, **cfg, wrt=("fluxes", "radec"))}


def tangent(a, fv, cfg, rng):
    g = _g(a, cfg, rng)
    db, dt = rng.normal(size=(len(cfg["baselines"]), 3)), rng.normal(size=(a.ntimes, np.size(cfg["ra"]), 3))
    head = {"array": a.array, "precision": cfg["precision"], "lib": os.environ.get("FFTVIS_HIP_LIB", "in-tree")}
    return head, {
        "forward": lambda: fv.simulate_vis(**cfg),
        "position": lambda: fv.simulate_vis_position_adjoint(g, **cfg, wrt="baselines"),
        "source": lambda: fv.simulate_vis_source_adjoint(g, **cfg, wrt="topo"),
        "tangent_baselines": lambda: fv.simulate_vis_jvp(**cfg, d_baselines=db),
        "tangent_directions": lambda: fv.simulate_vis_jvp(**cfg, d_topo=dt),
        "tangent_both": lambda: fv.simulate_vis_jvp(**cfg, d_baselines=db, d_topo=dt)}


def basis_tangent(a, fv, cfg, rng):
    g = _g(a, cfg, rng, cast=True)
    shape = (a.ndir,) + np.shape(cfg["beam_coefs"])
    d = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(g.dtype)
    head = {"config": a.config, "nbasis": len(cfg["beam"]), "precision": cfg["precision"], "ndir": a.ndir}
    return head, {
        "forward": lambda: fv.simulate_vis(**cfg),
        "tangent_1": lambda: fv.simulate_vis_basis_jvp(**cfg, d_beam_coefs=d[0]),
        "tangent_n": lambda: fv.simulate_vis_basis_jvp(**cfg, d_beam_coefs=d),
        "beam_coefs": lambda: fv.simulate_vis_basis_adjoint(g, **cfg, wrt="beam_coefs")}


def basis_position(a, fv, cfg, rng):
    g = _g(a, cfg, rng, cast=True)
    db = rng.normal(size=(len(cfg["baselines"]), 3))
    return {"config": a.config, "nbasis": len(cfg["beam"]), "precision": cfg["precision"]}, {
        "forward": lambda: fv.simulate_vis(**cfg),
        "adjoint": lambda: fv.simulate_vis_basis_adjoint(g, **cfg, wrt="baselines"),
        "tangent": lambda: fv.simulate_vis_basis_jvp(**cfg, d_baselines=db)}


def basis_source(a, fv, cfg, rng):
    if a.precision == 2:  # C5 is fp32 at eps 1e-4: its fp64 variant at the fp64 default of the benchmark configurations
        cfg.update(precision=2, eps=6e-8)
    g = _g(a, cfg, rng, cast=True)
    da = rng.normal(size=(len(cfg["ants"]), 3))
    dt = rng.normal(size=(a.ntimes, np.size(cfg["ra"]), 3))
    return {"config": a.config, "nbasis": len(cfg["beam"]), "precision": cfg["precision"]}, {
        "forward": lambda: fv.simulate_vis(**cfg),
        "fluxes": lambda: fv.simulate_vis_basis_adjoint(g, **cfg, wrt="fluxes"),
        "tangent_ants": lambda: fv.simulate_vis_basis_jvp(**cfg, d_ants=da),
        "source_adjoint": lambda: fv.simulate_vis_basis_source_adjoint(g, **cfg, wrt="topo"),
        "source_tangent": lambda: fv.simulate_vis_basis_source_jvp(**cfg, d_topo=dt),
        "joint": lambda: fv.simulate_vis_basis_sky_adjoint(g, **cfg, wrt=("fluxes", "topo"))}


def objective(a, fv, cfg, rng):
    if a.lattice:
        cfg["force_use_type3"] = False
    names = tuple(a.wrt.split(","))
    basis = cfg.get("beam_coefs") is not None
    p = cfg["precision"]
    cdt, rdt = (np.complex64, np.float32) if p == 1 else (np.complex128, np.float64)
    nbls = len(cfg["baselines"])
    shape = (a.nfreq, a.ntimes, 2, 2, nbls) if cfg["polarized"] else (a.nfreq, a.ntimes, nbls)
    d = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(cdt)
    w = rng.uniform(0.5, 2.0, size=shape).astype(rdt)
    sky = tuple(n for n in names if n in ("fluxes", "topo", "radec"))
    rest = tuple(n for n in names if n not in sky)

    def separate():
        g = (2 * w * (fv.simulate_vis(**cfg) - d)).astype(cdt)
        out = []
        if sky:
            out.append((fv.simulate_vis_basis_sky_adjoint if basis else fv.simulate_vis_sky_adjoint)(g, **cfg, wrt=sky))
        if rest:
            out.append((fv.simulate_vis_basis_adjoint if basis else fv.simulate_vis_position_adjoint)(g, **cfg, wrt=rest))
        return out

    calls = {"forward": lambda: fv.simulate_vis(**cfg), "separate": separate}
    gains = {}
    if a.gains:  # per-antenna gains 1 + 0.1 N(0, 1), constant in time; "gains" may be one of --wrt's names
        nant, nums = len(cfg["ants"]), list(cfg["ants"])
        gshape = (nant, 2, a.nfreq) if cfg["polarized"] else (nant, a.nfreq)
        g0 = (1 + 0.1 * (rng.normal(size=gshape) + 1j * rng.normal(size=gshape))).astype(cdt)
        gains = {"gains": g0}
        a1 = [nums.index(b[0]) for b in cfg["baselines"]]
        a2 = [nums.index(b[1]) for b in cfg["baselines"]]
        sky = tuple(n for n in sky if n != "gains")
        rest = tuple(n for n in rest if n != "gains")

        def separate():  # what a caller composes without gains=: the forward to the host, the gain product and the loss in
            # torch, .backward() for d chi2 / dV and the gain gradient, then the public adjoints on the host result
            import torch

            V = torch.from_numpy(fv.simulate_vis(**cfg)).cuda().requires_grad_(True)
            G = torch.from_numpy(g0).cuda().requires_grad_("gains" in names)
            D, W = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()
            g1, g2 = G[a1].conj(), G[a2]  # (nbls, [2,] nf)
            if cfg["polarized"]:  # out[f, t, x, y, k]: y is the first antenna's feed
                m = (g2.permute(2, 1, 0)[:, :, None, :] * g1.permute(2, 1, 0)[:, None, :, :])[:, None]
            else:
                m = (g1 * g2).T[:, None]
            (W * (m * V - D).abs() ** 2).sum().backward()
            g = V.grad.cpu().numpy()
            out = [G.grad]
            if sky:
                out.append((fv.simulate_vis_basis_sky_adjoint if basis else fv.simulate_vis_sky_adjoint)(g, **cfg, wrt=sky))
            if rest:
                out.append((fv.simulate_vis_basis_adjoint if basis else fv.simulate_vis_position_adjoint)(g, **cfg, wrt=rest))
            return out

        calls["separate"] = separate
        if a.profile == "gain_kernels":  # (for a kernel trace only) the gain kernels and k_residual_rows alone, alternating
            def gain_kernels():
                import importlib

                _lib = importlib.import_module(fv.__name__ + "._lib")
                lib = _lib.lib()
                rows, tpol = a.nfreq * a.ntimes, 4 if cfg["polarized"] else 1
                nfeed = 2 if cfg["polarized"] else 1
                gb = np.ascontiguousarray(np.broadcast_to(g0.reshape(nant, nfeed, a.nfreq, 1), (nant, nfeed, a.nfreq, a.ntimes))
                                          .transpose(2, 3, 1, 0))
                i1, i2 = np.array(a1, np.int32), np.array(a2, np.int32)
                v0 = (rng.normal(size=(rows, tpol * nbls)) + 1j * rng.normal(size=(rows, tpol * nbls))).astype(cdt)
                d2, w2, q, gg = d.reshape(rows, -1), w.reshape(rows, -1), np.zeros(rows), np.zeros(gb.shape, np.complex128)
                for _ in range(6):
                    v = v0.copy()
                    _lib.check(lib.fv_gain_residual_chi2(0, p, rows, nbls, tpol, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(gb),
                                                         _lib.ptr(v), _lib.ptr(d2), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(gg)))
                    v = v0.copy()
                    _lib.check(lib.fv_residual_chi2(0, p, rows, tpol * nbls, _lib.ptr(v), _lib.ptr(d2), _lib.ptr(w2), _lib.ptr(q)))

            calls["gain_kernels"] = gain_kernels
    if a.jones:  # one 2 x 2 matrix per antenna, identity + 0.1 N(0, 1), constant in time; "jones" may be one of --wrt's names
        nant, nums = len(cfg["ants"]), list(cfg["ants"])
        j0 = 0.1 * (rng.normal(size=(nant, 2, 2, a.nfreq)) + 1j * rng.normal(size=(nant, 2, 2, a.nfreq)))
        j0[:, 0, 0] += 1
        j0[:, 1, 1] += 1
        gains = {"jones": j0.astype(cdt)}
        a1 = [nums.index(b[0]) for b in cfg["baselines"]]
        a2 = [nums.index(b[1]) for b in cfg["baselines"]]
        del calls["separate"]  # (no composition to compare with: the diagonal gains' is --gains)
        if a.profile == "jones_kernels":  # (for a kernel trace only) the Jones kernels next to the gain kernels and
            # k_residual_rows alone, alternating, on host-uploaded blocks of the run's shape
            def jones_kernels():
                import importlib

                _lib = importlib.import_module(fv.__name__ + "._lib")
                lib = _lib.lib()
                rows = a.nfreq * a.ntimes
                jb = np.ascontiguousarray(np.broadcast_to(gains["jones"][..., None], (nant, 2, 2, a.nfreq, a.ntimes))
                                          .transpose(3, 4, 1, 2, 0))
                gb = np.ascontiguousarray(np.stack([jb[:, :, 0, 0], jb[:, :, 1, 1]], axis=2))
                i1, i2 = np.array(a1, np.int32), np.array(a2, np.int32)
                v0 = (rng.normal(size=(rows, 4 * nbls)) + 1j * rng.normal(size=(rows, 4 * nbls))).astype(cdt)
                d2, w2, q = d.reshape(rows, -1), w.reshape(rows, -1), np.zeros(rows)
                gj, gg = np.zeros(jb.shape, np.complex128), np.zeros(gb.shape, np.complex128)
                for _ in range(6):
                    v = v0.copy()
                    _lib.check(lib.fv_jones_residual_chi2(0, p, rows, nbls, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(jb),
                                                          _lib.ptr(v), _lib.ptr(d2), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(gj)))
                    v = v0.copy()
                    _lib.check(lib.fv_gain_residual_chi2(0, p, rows, nbls, 4, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(gb),
                                                         _lib.ptr(v), _lib.ptr(d2), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(gg)))
                    v = v0.copy()
                    _lib.check(lib.fv_residual_chi2(0, p, rows, 4 * nbls, _lib.ptr(v), _lib.ptr(d2), _lib.ptr(w2), _lib.ptr(q)))

            calls["jones_kernels"] = jones_kernels
    if names == ("fluxes",) and not basis and not a.gains and not a.jones:
        def separate_torch():
            import torch

            kw = {k: v for k, v in cfg.items() if k != "fluxes"}
            F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda", requires_grad=True)
            D, W = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()
            loss = (W * (fv.torch_simulate_vis(F, **kw) - D).abs() ** 2).sum()
            loss.backward()
            torch.cuda.synchronize()
            return F.grad

        calls["separate_torch"] = separate_torch
    if hasattr(fv, "simulate_vis_chi2"):
        resident = []

        def fused_device():
            import torch

            if not resident:
                resident.extend((torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()))
                if gains:
                    resident.append(torch.from_numpy(next(iter(gains.values()))).cuda())
                torch.cuda.synchronize()
            if a.jones:
                return fv.simulate_vis_jones_chi2(resident[0], **cfg, weights=resident[1], wrt=names, jones=resident[2])
            if gains:
                return fv.simulate_vis_gain_chi2(resident[0], **cfg, weights=resident[1], wrt=names, gains=resident[2])
            return fv.simulate_vis_chi2(resident[0], **cfg, weights=resident[1], wrt=names)

        chi2_call = fv.simulate_vis_jones_chi2 if a.jones else fv.simulate_vis_gain_chi2 if gains else fv.simulate_vis_chi2
        calls["fused"] = lambda: chi2_call(d, **cfg, weights=w, wrt=names, **gains)
        calls["fused_device"] = fused_device
    head = {"config": a.config, "precision": p, "polarized": bool(cfg["polarized"]), "lattice": bool(a.lattice), "wrt": list(names),
            "gains": bool(a.gains), "jones": bool(a.jones),
            # per call, from the shapes: V to the host and G back / d and w to the device / the gradients and chi2 alone
            "pcie_bytes": {"separate": 2 * d.nbytes, "fused": d.nbytes + w.nbytes, "fused_device": 0},
            "vis_bytes": d.nbytes}
    return head, calls


GAUSS_NEWTON_CASES = {"fluxes": ("fluxes",), "ants": ("ants",), "fluxes_radec": ("fluxes", "radec"), "beam_coefs": ("beam_coefs",),
                      "gains": (), "jones": ()}  # (no sky direction: --gains --d-gains, --jones --d-jones)


def gauss_newton(a, fv, cfg, rng):
    names = GAUSS_NEWTON_CASES[a.case]
    basis = cfg.get("beam_coefs") is not None
    if "radec" in names:
        cfg["coord_method"] = "SiderealRotation"
    p = cfg["precision"]
    cdt, rdt = (np.complex64, np.float32) if p == 1 else (np.complex128, np.float64)
    nbls = len(cfg["baselines"])
    shape = (a.nfreq, a.ntimes, 2, 2, nbls) if cfg["polarized"] else (a.nfreq, a.ntimes, nbls)
    w = rng.uniform(0.5, 2.0, size=shape).astype(rdt)
    F = np.asarray(cfg["fluxes"])
    dirs = {}
    if "fluxes" in names:
        dirs["d_fluxes"] = F * 0.3 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1))
    if "ants" in names:
        dirs["d_ants"] = 1e-2 * rng.normal(size=(len(cfg["ants"]), 3))
    if "radec" in names:
        dirs["d_radec"] = 1e-3 * rng.normal(size=(F.shape[0], 2))
    if "beam_coefs" in names:
        c = np.shape(cfg["beam_coefs"])
        dirs["d_beam_coefs"] = (0.1 * (rng.normal(size=c) + 1j * rng.normal(size=c))).astype(cdt)
    sky = tuple(n for n in names if n in ("fluxes", "radec"))
    rest = tuple(n for n in names if n not in sky)

    def composed():  # the two public calls: the tangent to the host, numpy's 2 w U, the adjoint on the host result
        # (quad is not formed: a conjugate-gradient caller has <p, H p> as a dot product of what it holds)
        u = (fv.simulate_vis_basis_jvp if basis else fv.simulate_vis_jvp)(**cfg, **dirs)
        g = (2 * w * u).astype(cdt)
        out = []
        if sky:
            out.append((fv.simulate_vis_basis_sky_adjoint if basis else fv.simulate_vis_sky_adjoint)(g, **cfg, wrt=sky))
        if rest:
            out.append((fv.simulate_vis_basis_adjoint if basis else fv.simulate_vis_position_adjoint)(g, **cfg, wrt=rest))
        return out

    calls = {"forward": lambda: fv.simulate_vis(**cfg), "composed": composed}
    gains = {}
    if a.d_gains and not a.gains:
        raise SystemExit("--d-gains needs --gains")
    if not names and not a.d_gains and not a.d_jones:
        raise SystemExit("--case gains needs --gains --d-gains, --case jones --jones --d-jones")
    if a.gains:
        nums = list(cfg["ants"])
        nant, nfeed = len(nums), 2 if cfg["polarized"] else 1
        gshape = ((nant, 2) if cfg["polarized"] else (nant,)) + (a.nfreq,)
        g0 = (1 + 0.1 * (rng.normal(size=gshape) + 1j * rng.normal(size=gshape))).astype(cdt)
        gains = {"gains": g0}
        if a.d_gains:
            gains["d_gains"] = (0.1 * (rng.normal(size=gshape) + 1j * rng.normal(size=gshape))).astype(cdt)
        a1 = [nums.index(b[0]) for b in cfg["baselines"]]
        a2 = [nums.index(b[1]) for b in cfg["baselines"]]
        out_names = names + (("gains",) if a.d_gains else ())

        def composed():  # what a caller composes without the new call: V and U to the host, the gain product, its tangent
            # and conj(m) 2 w U' in torch on the device, the public adjoint on the host result, the antennas' sums in torch
            import torch

            def product(x, y):  # conj(x[a1]) y[a2] in the block's shape
                x1, y2 = x[a1].conj(), y[a2]  # (nbls, [2,] nf)
                if cfg["polarized"]:  # out[f, t, x, y, k]: y is the first antenna's feed
                    return (y2.permute(2, 1, 0)[:, :, None, :] * x1.permute(2, 1, 0)[:, None, :, :])[:, None]
                return (x1 * y2).T[:, None]

            G0, W = torch.from_numpy(g0).cuda(), torch.from_numpy(w).cuda()
            m = product(G0, G0)
            up = 0
            if dirs:
                up = m * torch.from_numpy((fv.simulate_vis_basis_jvp if basis else fv.simulate_vis_jvp)(**cfg, **dirs)).cuda()
            out = []
            if a.d_gains:
                V = torch.from_numpy(fv.simulate_vis(**cfg)).cuda()
                H = torch.from_numpy(gains["d_gains"]).cuda()
                up = up + (product(H, G0) + product(G0, H)) * V
            gp = 2 * W * up
            if a.d_gains:  # the antennas' sums of conj(G') g2 V (first antenna's feed y) and G' g1 conj(V) (second's, x)
                hg = torch.zeros((nant, nfeed, a.nfreq), dtype=torch.complex128, device="cuda")
                i1, i2 = torch.tensor(a1, device="cuda"), torch.tensor(a2, device="cuda")
                g1, g2 = G0[a1], G0[a2]
                if cfg["polarized"]:
                    first = (gp.conj() * V * g2.permute(2, 1, 0)[:, None, :, None, :]).sum(dim=(1, 2))   # (f, y, k)
                    second = (gp * V.conj() * g1.permute(2, 1, 0)[:, None, None, :, :]).sum(dim=(1, 3))  # (f, x, k)
                    hg.index_add_(0, i1, first.permute(2, 1, 0).to(torch.complex128))
                    hg.index_add_(0, i2, second.permute(2, 1, 0).to(torch.complex128))
                else:
                    first, second = (gp.conj() * V * g2.T[:, None]).sum(dim=1), (gp * V.conj() * g1.T[:, None]).sum(dim=1)
                    hg[:, 0].index_add_(0, i1, first.T.to(torch.complex128))
                    hg[:, 0].index_add_(0, i2, second.T.to(torch.complex128))
                out.append(hg.cpu().numpy())
            g = (m.conj() * gp).cpu().numpy().astype(cdt)
            if sky:
                out.append((fv.simulate_vis_basis_sky_adjoint if basis else fv.simulate_vis_sky_adjoint)(g, **cfg, wrt=sky))
            if rest:
                out.append((fv.simulate_vis_basis_adjoint if basis else fv.simulate_vis_position_adjoint)(g, **cfg, wrt=rest))
            return out

        calls["composed"] = composed
        if a.profile == "gain_kernels":  # (for a kernel trace only) the gain weighting kernels next to k_weight_rows and the
            # objective's gain kernels, alone on the block's shape, alternating
            def gain_kernels():
                import ctypes
                import importlib

                _lib = importlib.import_module(fv.__name__ + "._lib")
                lib = _lib.lib()
                rows, tpol = a.nfreq * a.ntimes, 4 if cfg["polarized"] else 1
                L = tpol * nbls

                def block(x):
                    return np.ascontiguousarray(np.broadcast_to(x.reshape(nant, nfeed, a.nfreq, 1), (nant, nfeed, a.nfreq, a.ntimes))
                                                .transpose(2, 3, 1, 0))

                gb = block(g0)
                hb = block(gains["d_gains"]) if a.d_gains else None
                i1, i2 = np.array(a1, np.int32), np.array(a2, np.int32)
                u = (rng.normal(size=(rows, L)) + 1j * rng.normal(size=(rows, L))).astype(cdt)
                v0, w2, q, hg = u[::-1].copy(), w.reshape(rows, L), np.zeros(rows), np.zeros(gb.shape, np.complex128)
                for _ in range(6):
                    part, v = u.copy(), v0.copy()
                    ptrs = (ctypes.c_void_p * 1)(part.ctypes.data)
                    _lib.check(lib.fv_gain_weight_rows(0, p, rows, nbls, tpol, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(gb),
                                                       _lib.ptr(hb), 1, ptrs, _lib.ptr(v), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(hg)))
                    part = u.copy()
                    ptrs = (ctypes.c_void_p * 1)(part.ctypes.data)
                    _lib.check(lib.fv_weight_rows(0, p, rows, L, 1, ptrs, _lib.ptr(w2), _lib.ptr(q)))
                    v = v0.copy()
                    _lib.check(lib.fv_gain_residual_chi2(0, p, rows, nbls, tpol, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(gb),
                                                         _lib.ptr(v), _lib.ptr(u), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(hg)))

            calls["gain_kernels"] = gain_kernels
    if a.d_jones and not a.jones:
        raise SystemExit("--d-jones needs --jones")
    if a.jones and a.gains:
        raise SystemExit("--jones or --gains, not both")
    if a.jones:  # one 2 x 2 matrix per antenna, identity + 0.1 N(0, 1), constant in time, and a direction of 0.1 N(0, 1)
        nums = list(cfg["ants"])
        nant = len(nums)
        jshape = (nant, 2, 2, a.nfreq)
        j0 = 0.1 * (rng.normal(size=jshape) + 1j * rng.normal(size=jshape))
        j0[:, 0, 0] += 1
        j0[:, 1, 1] += 1
        gains = {"jones": j0.astype(cdt)}
        if a.d_jones:
            gains["d_jones"] = (0.1 * (rng.normal(size=jshape) + 1j * rng.normal(size=jshape))).astype(cdt)
        a1 = [nums.index(b[0]) for b in cfg["baselines"]]
        a2 = [nums.index(b[1]) for b in cfg["baselines"]]
        out_names = names + (("jones",) if a.d_jones else ())

        def jones_block(x):  # (nf, nt, 2, 2, nant)
            return np.ascontiguousarray(np.broadcast_to(x[..., None], jshape + (a.ntimes,)).transpose(3, 4, 1, 2, 0))

        def composed():  # what a caller composes without the new call: U and, with --d-jones, V to the host, the 2 x 2
            # products, 2 w U', the transposed product and the antennas' sums in numpy, the public adjoint on the host result
            def product(x, ga, gb):  # sum conj(ga[a1][y', y]) gb[a2][x', x] x[x', y']
                return np.einsum("...bdk,...ack,...abk->...cdk", np.conj(ga[..., a1]), gb[..., a2], x)

            jb = jones_block(gains["jones"])
            up = 0
            if dirs:
                up = product((fv.simulate_vis_basis_jvp if basis else fv.simulate_vis_jvp)(**cfg, **dirs), jb, jb)
            out = []
            if a.d_jones:
                v = fv.simulate_vis(**cfg)
                hb = jones_block(gains["d_jones"])
                up = up + product(v, hb, jb) + product(v, jb, hb)
            gp = 2 * w * up
            g1, g2 = jb[..., a1], jb[..., a2]
            if a.d_jones:  # the antennas' sums of the two sides
                hj = np.zeros(jb.shape, dtype=np.complex128)
                m = np.einsum("...ack,...abk->...cbk", g2, v)
                np.add.at(hj, (Ellipsis, a1), np.einsum("...cdk,...cbk->...bdk", np.conj(gp), m))
                b = np.einsum("...abk,...bdk->...adk", v, np.conj(g1))
                np.add.at(hj, (Ellipsis, a2), np.einsum("...cdk,...adk->...ack", gp, np.conj(b)))
                out.append(hj.sum(axis=1).transpose(3, 1, 2, 0))
            g = np.einsum("...ack,...cdk,...bdk->...abk", np.conj(g2), gp, g1).astype(cdt)
            if sky:
                out.append((fv.simulate_vis_basis_sky_adjoint if basis else fv.simulate_vis_sky_adjoint)(g, **cfg, wrt=sky))
            if rest:
                out.append((fv.simulate_vis_basis_adjoint if basis else fv.simulate_vis_position_adjoint)(g, **cfg, wrt=rest))
            return out

        calls["composed"] = composed
        if hasattr(fv, "simulate_vis_gain_gauss_newton"):  # the diagonal of the same matrices, in the same job
            diag = {k.replace("jones", "gains"): np.ascontiguousarray(np.stack([v[:, 0, 0], v[:, 1, 1]], axis=1))
                    for k, v in gains.items()}
            gain_names = names + (("gains",) if a.d_jones else ())
            resident_w = []

            def gain_fused_device():
                import torch

                if not resident_w:
                    resident_w.append(torch.from_numpy(w).cuda())
                    torch.cuda.synchronize()
                return fv.simulate_vis_gain_gauss_newton(**cfg, **dirs, **diag, weights=resident_w[0], wrt=gain_names)

            calls["gain_fused_device"] = gain_fused_device
        if a.profile == "jones_kernels":  # (for a kernel trace only) the Jones weighting kernels next to the gain weighting
            # kernels (the diagonal of the same matrices) and k_weight_rows, alone on the block's shape, alternating
            def jones_kernels():
                import ctypes
                import importlib

                _lib = importlib.import_module(fv.__name__ + "._lib")
                lib = _lib.lib()
                rows, L = a.nfreq * a.ntimes, 4 * nbls
                jb = jones_block(gains["jones"]).reshape(rows, 2, 2, nant)
                hb = jones_block(gains["d_jones"]).reshape(rows, 2, 2, nant) if a.d_jones else None
                gb = np.ascontiguousarray(np.stack([jb[:, 0, 0], jb[:, 1, 1]], axis=1))
                dgb = np.ascontiguousarray(np.stack([hb[:, 0, 0], hb[:, 1, 1]], axis=1)) if a.d_jones else None
                i1, i2 = np.array(a1, np.int32), np.array(a2, np.int32)
                u = (rng.normal(size=(rows, L)) + 1j * rng.normal(size=(rows, L))).astype(cdt)
                v0, w2, q = u[::-1].copy(), w.reshape(rows, L), np.zeros(rows)
                hj, hg = np.zeros(jb.shape, np.complex128), np.zeros(gb.shape, np.complex128)
                for _ in range(6):
                    part, v = u.copy(), v0.copy()
                    ptrs = (ctypes.c_void_p * 1)(part.ctypes.data)
                    _lib.check(lib.fv_jones_weight_rows(0, p, rows, nbls, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(jb),
                                                        _lib.ptr(hb), 1, ptrs, _lib.ptr(v), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(hj)))
                    part, v = u.copy(), v0.copy()
                    ptrs = (ctypes.c_void_p * 1)(part.ctypes.data)
                    _lib.check(lib.fv_gain_weight_rows(0, p, rows, nbls, 4, nant, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(gb),
                                                       _lib.ptr(dgb), 1, ptrs, _lib.ptr(v), _lib.ptr(w2), _lib.ptr(q), _lib.ptr(hg)))
                    part = u.copy()
                    ptrs = (ctypes.c_void_p * 1)(part.ctypes.data)
                    _lib.check(lib.fv_weight_rows(0, p, rows, L, 1, ptrs, _lib.ptr(w2), _lib.ptr(q)))

            calls["jones_kernels"] = jones_kernels
    if a.profile == "kernels":  # (for a kernel trace only) the two streaming kernels alone on the block's shape, alternating
        def kernels():
            import ctypes
            import importlib

            _lib = importlib.import_module(fv.__name__ + "._lib")
            lib = _lib.lib()
            rows, L = a.nfreq * a.ntimes, w.size // (a.nfreq * a.ntimes)
            u = (rng.normal(size=(rows, L)) + 1j * rng.normal(size=(rows, L))).astype(cdt)
            d, w2, q = u[::-1].copy(), w.reshape(rows, L), np.zeros(rows)
            for _ in range(6):
                part = u.copy()
                ptrs = (ctypes.c_void_p * 1)(part.ctypes.data)
                _lib.check(lib.fv_weight_rows(0, p, rows, L, 1, ptrs, _lib.ptr(w2), _lib.ptr(q)))
                g = u.copy()
                _lib.check(lib.fv_residual_chi2(0, p, rows, L, _lib.ptr(g), _lib.ptr(d), _lib.ptr(w2), _lib.ptr(q)))

        calls["kernels"] = kernels
    if hasattr(fv, "simulate_vis_gauss_newton"):
        resident = []

        def fused_device():
            import torch

            if not resident:
                resident.append(torch.from_numpy(w).cuda())
                torch.cuda.synchronize()
            if gains:
                return with_gains(**cfg, **dirs, **gains, weights=resident[0], wrt=out_names)
            return fv.simulate_vis_gauss_newton(**cfg, **dirs, weights=resident[0], wrt=names)

        if a.jones and not hasattr(fv, "simulate_vis_jones_gauss_newton"):
            pass  # (a checkout from before the call has ``composed`` and ``gain_fused_device`` alone)
        elif gains:
            with_gains = fv.simulate_vis_jones_gauss_newton if a.jones else fv.simulate_vis_gain_gauss_newton
            calls["fused"] = lambda: with_gains(**cfg, **dirs, **gains, weights=w, wrt=out_names)
            calls["fused_device"] = fused_device
        else:
            calls["fused"] = lambda: fv.simulate_vis_gauss_newton(**cfg, **dirs, weights=w, wrt=names)
            calls["fused_device"] = fused_device
    vis_bytes = w.size * np.dtype(cdt).itemsize
    head = {"config": a.config, "case": a.case, "precision": p, "polarized": bool(cfg["polarized"]), "wrt": list(names),
            "gains": bool(a.gains), "d_gains": bool(a.d_gains), "jones": bool(a.jones), "d_jones": bool(a.d_jones),
            # per call, from the shapes: U to the host and G back / w to the device / the directions and products alone
            "pcie_bytes": {"composed": 2 * vis_bytes, "fused": w.nbytes, "fused_device": 0}, "vis_bytes": vis_bytes}
    return head, calls


GAIN_SOLVE_ITERATIONS = 50


def gain_solve(a, fv, cfg, rng):
    """The gains-only solve against a fixed model: GAIN_SOLVE_ITERATIONS iterations of ``simulate_vis_gain_solve`` on a
    resident model with resident data and weights (host to host: the gains go up and come back), next to as many gains-only
    products of ``simulate_vis_gain_gauss_newton(d_gains=...)`` -- what an iteration of such a solve costs without it, every
    call rerunning the forward.  ``--profile solve`` is one solve on a resident model, for a kernel trace (the forward and the
    one-iteration solve that make the model are the only other work of the process)."""
    import torch

    p = cfg["precision"]
    cdt, rdt = (np.complex64, np.float32) if p == 1 else (np.complex128, np.float64)
    nums = list(cfg["ants"])
    nant = len(nums)
    gshape = ((nant, 2) if cfg["polarized"] else (nant,)) + (a.nfreq,)
    g_true = 1 + 0.1 * (rng.normal(size=gshape) + 1j * rng.normal(size=gshape))
    d_gains = (0.1 * (rng.normal(size=gshape) + 1j * rng.normal(size=gshape))).astype(cdt)
    state = {}

    def resident():  # the model from one forward, data = the gained model plus noise, the cross-hands flagged
        if not state:
            _, _, model = fv.simulate_vis_gain_solve(_zeros_like_vis(), **cfg, max_iter=1, tol=0.0, return_model=True)
            G = torch.from_numpy(g_true).cuda()
            a1 = torch.tensor([nums.index(b[0]) for b in cfg["baselines"]], device="cuda")
            a2 = torch.tensor([nums.index(b[1]) for b in cfg["baselines"]], device="cuda")
            if cfg["polarized"]:  # out[f, t, x, y, k]: y is the first antenna's feed
                m = (G[a2].permute(2, 1, 0)[:, :, None, :] * G[a1].conj().permute(2, 1, 0)[:, None, :, :])[:, None]
            else:
                m = (G[a1].conj() * G[a2]).T[:, None]
            data = m * model
            noise = 0.05 * data.abs().mean()
            data = (data + noise * torch.randn_like(data)).to(model.dtype)
            w = torch.ones(model.shape, dtype=getattr(torch, np.dtype(rdt).name), device="cuda")
            if cfg["polarized"]:
                w[:, :, 0, 1] = 0
                w[:, :, 1, 0] = 0
            torch.cuda.synchronize()
            state.update(model=model, data=data, w=w)
        return state

    def _zeros_like_vis():
        nbls = len(cfg["baselines"])
        return np.zeros((a.nfreq, a.ntimes, 2, 2, nbls) if cfg["polarized"] else (a.nfreq, a.ntimes, nbls), dtype=cdt)

    def solve():
        s = resident()
        return fv.simulate_vis_gain_solve(s["data"], **dict(cfg, fluxes=None), weights=s["w"], model=s["model"],
                                          max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def solve_with_forward():  # the same from the sky: one forward, then the iterations
        s = resident()
        return fv.simulate_vis_gain_solve(s["data"], **cfg, weights=s["w"], max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def products():
        s = resident()
        g = np.ones(gshape, dtype=cdt)
        for _ in range(GAIN_SOLVE_ITERATIONS):
            fv.simulate_vis_gain_gauss_newton(**cfg, gains=g, d_gains=d_gains, weights=s["w"], wrt="gains")

    calls = {"forward": lambda: fv.simulate_vis(**cfg), "solve": solve, "solve_with_forward": solve_with_forward,
             "gauss_newton_products": products}
    head = {"config": a.config, "precision": p, "polarized": bool(cfg["polarized"]), "iterations": GAIN_SOLVE_ITERATIONS}
    return head, calls


def jones_solve(a, fv, cfg, rng):
    """The Jones solve against a fixed model: GAIN_SOLVE_ITERATIONS iterations of ``simulate_vis_jones_solve`` on a resident
    model with resident data and weights (host to host: the matrices go up and come back), next to as many steps of what
    such a fit costs without it, ``simulate_vis_jones_chi2`` with its gradient, each of which reruns the forward.  No sample
    is flagged: the solve uses the cross-hands.  ``--profile solve`` is one solve on a resident model, for a kernel trace."""
    import torch

    p = cfg["precision"]
    cdt, rdt = (np.complex64, np.float32) if p == 1 else (np.complex128, np.float64)
    nums = list(cfg["ants"])
    nant = len(nums)
    jshape = (nant, 2, 2, a.nfreq)
    j_true = 0.1 * (rng.normal(size=jshape) + 1j * rng.normal(size=jshape))
    j_true[:, 0, 0] += 1
    j_true[:, 1, 1] += 1
    state = {}

    def resident():  # the model from one forward, data = the model under the true matrices plus noise
        if not state:
            nbls = len(cfg["baselines"])
            zeros = np.zeros((a.nfreq, a.ntimes, 2, 2, nbls), dtype=cdt)
            _, _, model = fv.simulate_vis_jones_solve(zeros, **cfg, max_iter=1, tol=0.0, return_model=True)
            G = torch.from_numpy(j_true).cuda()  # [a, i, j, f]
            a1 = torch.tensor([nums.index(b[0]) for b in cfg["baselines"]], device="cuda")
            a2 = torch.tensor([nums.index(b[1]) for b in cfg["baselines"]], device="cuda")
            # V'[f, t, x, y, k] = sum conj(G1[y', y]) G2[x', x] V[x', y']
            data = torch.einsum("kbdf,kacf,ftabk->ftcdk", G[a1].conj(), G[a2], model.to(G.dtype))
            noise = 0.05 * data.abs().mean()
            data = (data + noise * torch.randn_like(data)).to(model.dtype).contiguous()
            w = torch.ones(model.shape, dtype=getattr(torch, np.dtype(rdt).name), device="cuda")
            torch.cuda.synchronize()
            state.update(model=model, data=data, w=w)
        return state

    def solve():
        s = resident()
        return fv.simulate_vis_jones_solve(s["data"], **dict(cfg, fluxes=None), weights=s["w"], model=s["model"],
                                           max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def solve_with_forward():  # the same from the sky: one forward, then the iterations
        s = resident()
        return fv.simulate_vis_jones_solve(s["data"], **cfg, weights=s["w"], max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def chi2_steps():
        s = resident()
        eye = np.zeros(jshape, dtype=cdt)
        eye[:, 0, 0] = eye[:, 1, 1] = 1
        for _ in range(GAIN_SOLVE_ITERATIONS):
            fv.simulate_vis_jones_chi2(s["data"], **cfg, jones=eye, weights=s["w"], wrt="jones")

    calls = {"forward": lambda: fv.simulate_vis(**cfg), "solve": solve, "solve_with_forward": solve_with_forward,
             "jones_chi2_steps": chi2_steps}
    head = {"config": a.config, "precision": p, "polarized": True, "iterations": GAIN_SOLVE_ITERATIONS}
    return head, calls


def redundant_solve(a, fv, cfg, rng):
    """Redundant calibration next to the gain solve on the same block: GAIN_SOLVE_ITERATIONS iterations of
    ``redundant_gain_solve`` on resident data and weights (host to host: the gains go up, the gains and the groups'
    visibilities come back), and as many of ``simulate_vis_gain_solve`` against the resident model ``U[group]``.  Every
    baseline of the array in group order, no sample flagged; the data are drawn group by group -- no forward runs.
    ``--profile both`` is one solve of each, for a kernel trace."""
    import torch

    p = cfg["precision"]
    cdt, rdt = (torch.complex64, torch.float32) if p == 1 else (torch.complex128, torch.float64)
    ants, polarized = cfg["ants"], bool(cfg["polarized"])
    nums = list(ants)
    reds, bls, group = fv.redundant_groups(ants)
    cfg = dict(cfg, baselines=bls, fluxes=None)
    gshape = ((len(nums), 2) if polarized else (len(nums),)) + (a.nfreq,)
    g_true = 1 + 0.1 * (rng.normal(size=gshape) + 1j * rng.normal(size=gshape))
    state = {}

    def resident():  # the model is every baseline's group visibility; data = the gained model plus noise
        if not state:
            gen = torch.Generator(device="cuda").manual_seed(0)
            U = torch.randn((a.nfreq, a.ntimes) + ((2, 2) if polarized else ()) + (len(reds),), dtype=torch.complex128,
                            device="cuda", generator=gen)
            model = U[..., torch.from_numpy(group).cuda().long()].to(cdt).contiguous()
            G = torch.from_numpy(g_true).cuda()
            a1 = torch.tensor([nums.index(b[0]) for b in bls], device="cuda")
            a2 = torch.tensor([nums.index(b[1]) for b in bls], device="cuda")
            if polarized:  # out[f, t, x, y, k]: y is the first antenna's feed
                m = (G[a2].permute(2, 1, 0)[:, :, None, :] * G[a1].conj().permute(2, 1, 0)[:, None, :, :])[:, None]
            else:
                m = (G[a1].conj() * G[a2]).T[:, None]
            data = m * model
            data = (data + 0.05 * data.abs().mean() * torch.randn(data.shape, dtype=data.dtype, device="cuda", generator=gen))
            state.update(model=model, data=data.to(cdt).contiguous(), w=torch.ones(model.shape, dtype=rdt, device="cuda"))
            torch.cuda.synchronize()
        return state

    def solve():
        s = resident()
        return fv.redundant_gain_solve(s["data"], ants, reds=reds, weights=s["w"], polarized=polarized,  # (bls: the default)
                                       precision=p, max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def gain_solve_on_the_block():
        s = resident()
        return fv.simulate_vis_gain_solve(s["data"], **cfg, weights=s["w"], model=s["model"], max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def both():
        solve()
        gain_solve_on_the_block()

    head = {"config": a.config, "precision": p, "polarized": polarized, "iterations": GAIN_SOLVE_ITERATIONS, "ngroups": len(reds)}
    return head, {"solve": solve, "gain_solve": gain_solve_on_the_block, "both": both}


def firstcal(a, fv, cfg, rng):
    """Firstcal on resident data and weights (host to host): ``redundant_firstcal`` with GAIN_SOLVE_ITERATIONS iterations of
    its second stage, and the ``redundant_gain_solve`` it starts, as many iterations from the firstcal gains.  Every baseline
    of the array in group order, no sample flagged, channels of 0.5 MHz; the gains carry delays uniform in +-150 ns, phases
    in +-pi and amplitudes 1 +- 0.1; the data are drawn group by group, 5 % noise -- no forward runs.  ``--profile firstcal``
    is one call, for a kernel trace."""
    import torch

    p = cfg["precision"]
    cdt, rdt = (torch.complex64, torch.float32) if p == 1 else (torch.complex128, torch.float64)
    ants, polarized = cfg["ants"], bool(cfg["polarized"])
    nums = list(ants)
    reds, bls, group = fv.redundant_groups(ants)
    cfg["baselines"] = bls  # (the line's nbls)
    freqs = 150e6 + 0.5e6 * np.arange(a.nfreq)
    lead = (len(nums), 2) if polarized else (len(nums),)
    tau = rng.uniform(-150e-9, 150e-9, lead)
    c = rng.uniform(0.9, 1.1, lead) * np.exp(1j * rng.uniform(-np.pi, np.pi, lead))
    g_true = c[..., None] * np.exp(2j * np.pi * tau[..., None] * (freqs - freqs.mean()))
    state = {}

    def resident():
        if not state:
            gen = torch.Generator(device="cuda").manual_seed(0)
            U = torch.randn((a.nfreq, a.ntimes) + ((2, 2) if polarized else ()) + (len(reds),), dtype=torch.complex128,
                            device="cuda", generator=gen)
            G = torch.from_numpy(g_true).cuda()
            a1 = torch.tensor([nums.index(b[0]) for b in bls], device="cuda")
            a2 = torch.tensor([nums.index(b[1]) for b in bls], device="cuda")
            if polarized:  # out[f, t, x, y, k]: y is the first antenna's feed
                m = (G[a2].permute(2, 1, 0)[:, :, None, :] * G[a1].conj().permute(2, 1, 0)[:, None, :, :])[:, None]
            else:
                m = (G[a1].conj() * G[a2]).T[:, None]
            data = m * U[..., torch.from_numpy(group).cuda().long()]
            data += 0.05 * torch.randn(data.shape, dtype=data.dtype, device="cuda", generator=gen)
            state.update(data=data.to(cdt).contiguous(), w=torch.ones(data.shape, dtype=rdt, device="cuda"))
            del data, m, U
            torch.cuda.synchronize()
        return state

    def first():
        s = resident()
        return fv.redundant_firstcal(s["data"], ants, freqs, reds=reds, weights=s["w"], polarized=polarized, precision=p,
                                     max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def solve():
        s = resident()
        if "gains" not in s:
            s["gains"] = first()[0]
        return fv.redundant_gain_solve(s["data"], ants, reds=reds, gains=s["gains"], weights=s["w"], polarized=polarized,
                                       precision=p, max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    head = {"config": a.config, "precision": p, "polarized": polarized, "iterations": GAIN_SOLVE_ITERATIONS, "ngroups": len(reds),
            "npairs": len(bls) - len(reds)}
    return head, {"firstcal": first, "solve": solve}


def abscal(a, fv, cfg, rng):
    """Abscal on resident group visibilities, model and weights (host to host: the gains go up and come back), next to the
    route to the same end through the sky: a forward on every baseline, ``simulate_vis_gain_solve`` (GAIN_SOLVE_ITERATIONS
    iterations against the resident model) and ``fix_redundant_degeneracies``.  The group visibilities are the model moved by
    a planted amplitude and slope per channel and feed, 5 % noise; the sky route's data and model are random blocks (its
    iterations do not depend on the values).  ``--profile abscal`` is one call, for a kernel trace."""
    import torch

    p = cfg["precision"]
    cdt, rdt = (torch.complex64, torch.float32) if p == 1 else (torch.complex128, torch.float64)
    ants, polarized = cfg["ants"], bool(cfg["polarized"])
    nant = len(ants)
    reds, bls, group = fv.redundant_groups(ants)
    pos = np.array([np.asarray(ants[k], float) for k in ants])
    b = np.array([pos[list(ants).index(r[0][1])] - pos[list(ants).index(r[0][0])] for r in reds])
    lead = (nant, 2) if polarized else (nant,)
    gains = np.ones(lead + (a.nfreq,), dtype=np.complex128)
    pol = (2, 2) if polarized else ()
    state = {}

    def resident():
        if not state:
            gen = torch.Generator(device="cuda").manual_seed(0)
            M = torch.randn((a.nfreq, a.ntimes) + pol + (len(reds),), dtype=torch.complex128, device="cuda", generator=gen)
            phi = rng.uniform(-0.3, 0.3, (a.nfreq, 1) + pol + (1, 3)) * np.pi / np.sqrt((b**2).sum(axis=1)).min() * [1, 1, 0]
            turn = torch.from_numpy(np.exp(1j * (phi * b).sum(axis=-1)) / rng.uniform(0.5, 2.0, (a.nfreq, 1) + pol + (1,))).cuda()
            vis = M * turn + 0.05 * torch.randn(M.shape, dtype=M.dtype, device="cuda", generator=gen)
            state.update(vis=vis.contiguous(), model=M.to(cdt).contiguous(), w=torch.ones(M.shape, dtype=torch.float64, device="cuda"))
            torch.cuda.synchronize()
        return state

    def sky():  # the sky route's blocks, every baseline
        if "data" not in state:
            gen = torch.Generator(device="cuda").manual_seed(1)
            shape = (a.nfreq, a.ntimes) + pol + (len(bls),)
            state.update(data=torch.randn(shape, dtype=cdt, device="cuda", generator=gen),
                         sky_model=torch.randn(shape, dtype=cdt, device="cuda", generator=gen), sky_w=torch.ones(shape, dtype=rdt, device="cuda"))
            torch.cuda.synchronize()
        return state

    def fit():
        s = resident()
        return fv.redundant_abscal(s["vis"], s["model"], ants, gains, reds=reds, weights=s["w"], polarized=polarized, precision=p)

    def gain_solve_all():
        s = sky()
        return fv.simulate_vis_gain_solve(s["data"], **dict(cfg, baselines=bls, fluxes=None), weights=s["sky_w"], model=s["sky_model"],
                                          max_iter=GAIN_SOLVE_ITERATIONS, tol=0.0)

    def fix():
        if "g_sky" not in state:
            state["g_sky"] = gains * np.exp(1j * rng.uniform(-0.5, 0.5, gains.shape))
        return fv.fix_redundant_degeneracies(gains, ants, ref_gains=state["g_sky"])

    calls = {"abscal": fit, "model_groups": lambda: fv.simulate_vis(**dict(cfg, baselines=[r[0] for r in reds])),
             "model_all": lambda: fv.simulate_vis(**dict(cfg, baselines=bls)), "gain_solve": gain_solve_all, "fix": fix}
    cfg["baselines"] = bls  # (the line's nbls)
    head = {"config": a.config, "precision": p, "polarized": polarized, "iterations": GAIN_SOLVE_ITERATIONS, "ngroups": len(reds)}
    return head, calls


# family: (its function, default --config, default --nfreq, its own flags, what goes with a median: "range" | "runs" | None,
#          ratios {key: (pass, pass it is divided by -- either may be a tuple of passes, for their sum)})
FAMILIES = {
    "adjoint": (adjoint, "C3", 2, ("lattice", "adjoint_path"), "range", {"adjoint_over_forward": ("adjoint", "forward")}),
    "basis_adjoint": (basis_adjoint, "C5", 4, ("small",), None, {}),
    "position": (position, "C3", 8, ("array",), "runs", {"position_over_forward": ("position", "forward")}),
    "source": (source, "C3", 8, (), "runs", {"sources_over_fluxes": ("sources", "fluxes"),
                                            "sources_over_forward": ("sources", "forward"),
                                            "joint_over_fluxes_plus_sources": ("joint", ("fluxes", "sources"))}),
    "tangent": (tangent, "C3", 8, ("array",), "runs", {}),
    "basis_tangent": (basis_tangent, "C5", 8, ("ndir",), "runs", {}),
    "basis_position": (basis_position, "C5", 8, (), "runs", {"adjoint_over_forward": ("adjoint", "forward"),
                                                            "tangent_over_forward": ("tangent", "forward")}),
    "basis_source": (basis_source, "C5", 8, ("precision",), "runs", {
        "source_adjoint_over_fluxes": ("source_adjoint", "fluxes"), "source_adjoint_over_forward": ("source_adjoint", "forward"),
        "source_tangent_over_forward": ("source_tangent", "forward"),
        "source_tangent_over_tangent_ants": ("source_tangent", "tangent_ants"),
        "joint_over_fluxes_plus_source_adjoint": ("joint", ("fluxes", "source_adjoint"))}),
    "objective": (objective, "C3", 8, ("lattice", "wrt", "gains", "jones"), "runs", {
        "separate_over_forward": ("separate", "forward"), "fused_over_separate": ("fused", "separate"),
        "fused_device_over_separate": ("fused_device", "separate"), "fused_device_over_forward": ("fused_device", "forward"),
        "separate_torch_over_separate": ("separate_torch", "separate")}),
    "gauss_newton": (gauss_newton, "C3", 8, ("case", "gains", "d_gains", "jones", "d_jones"), "runs", {
        "composed_over_forward": ("composed", "forward"), "fused_over_composed": ("fused", "composed"),
        "fused_device_over_composed": ("fused_device", "composed"), "fused_device_over_forward": ("fused_device", "forward"),
        "fused_device_over_gain_fused_device": ("fused_device", "gain_fused_device")}),
    "gain_solve": (gain_solve, "C3", 8, (), "runs", {
        "solve_over_forward": ("solve", "forward"), "products_over_solve": ("gauss_newton_products", "solve")}),
    "jones_solve": (jones_solve, "C3", 8, (), "runs", {
        "solve_over_forward": ("solve", "forward"), "chi2_steps_over_solve": ("jones_chi2_steps", "solve")}),
    "redundant_solve": (redundant_solve, "C3", 8, (), "runs", {"solve_over_gain_solve": ("solve", "gain_solve")}),
    "firstcal": (firstcal, "C3", 8, (), "runs", {"firstcal_over_solve": ("firstcal", "solve")}),
    "abscal": (abscal, "C3", 8, (), "runs", {"abscal_route_over_sky_route": (("abscal", "model_groups"), ("model_all", "gain_solve", "fix"))}),
}
OWN_FLAGS = {"array": "ideal", "lattice": False, "adjoint_path": "type3", "small": False, "ndir": 8,
             "precision": 1, "wrt": "fluxes", "case": "fluxes", "gains": False, "d_gains": False, "jones": False,
             "d_jones": False}  # and their defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=list(FAMILIES), required=True)
    ap.add_argument("--config", default=None)
    ap.add_argument("--nsrc", type=int, default=None)
    ap.add_argument("--nfreq", type=int, default=None)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", action="append", default=None, metavar="PASS")
    ap.add_argument("--profile", default=None, metavar="PASS")
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose fftvis_amd is measured (default: this one)")
    ap.add_argument("--array", choices=["ideal", "surveyed"], default=None)
    ap.add_argument("--lattice", action="store_true", default=None, help="force_use_type3=False: the type-1 forward")
    ap.add_argument("--adjoint-path", choices=["type3", "type2", "auto"], default=None)
    ap.add_argument("--small", action="store_true", default=None, help="HERA-37, K = 3 Airy dishes, fp64")
    ap.add_argument("--ndir", type=int, default=None)
    ap.add_argument("--wrt", default=None, help="objective: the gradients, comma-separated (default fluxes)")
    ap.add_argument("--gains", action="store_true", default=None,
                    help="objective: per-antenna gains in the data model (gains may then be one of --wrt's names); "
                         "gauss_newton: the gains in the data model (simulate_vis_gain_gauss_newton)")
    ap.add_argument("--jones", action="store_true", default=None,
                    help="objective: one 2 x 2 matrix per antenna in the data model (simulate_vis_jones_chi2; jones may then "
                         "be one of --wrt's names; a polarized configuration); gauss_newton: the matrices in the data model "
                         "(simulate_vis_jones_gauss_newton)")
    ap.add_argument("--d-gains", action="store_true", default=None,
                    help="gauss_newton, with --gains: a gain direction, and the gain block among the products")
    ap.add_argument("--d-jones", action="store_true", default=None,
                    help="gauss_newton, with --jones: a direction of 2 x 2 matrices, and the matrices' block among the products")
    ap.add_argument("--precision", type=int, choices=[1, 2], default=None, help="2: the configuration in fp64 at eps 6e-8")
    ap.add_argument("--case", choices=list(GAUSS_NEWTON_CASES), default=None,
                    help="gauss_newton: the direction and the products (default fluxes; beam_coefs: --config C5; gains: no "
                         "sky direction, with --gains --d-gains)")
    a = ap.parse_args()
    build, config, nfreq, own, spread, ratios = FAMILIES[a.family]
    for flag, default in OWN_FLAGS.items():
        if flag not in own and getattr(a, flag) is not None:
            ap.error(f"--{flag.replace('_', '-')} does not apply to --family {a.family}")
        if getattr(a, flag) is None:
            setattr(a, flag, default)
    a.config, a.nfreq = a.config or config, a.nfreq or nfreq
    sys.path.insert(0, os.path.abspath(a.package))
    import fftvis_amd as fv
    from fftvis_amd import synth  # noqa: F401  (fv.synth)

    cfg = small_basis_config(fv, a.nfreq, a.ntimes) if a.small else synth.make_config(a.config, nsrc=a.nsrc, nfreq=a.nfreq,
                                                                                      ntimes=a.ntimes)
    if a.array == "surveyed":
        cfg["ants"] = surveyed(cfg["ants"])
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    head, calls = build(a, fv, cfg, np.random.default_rng(0))
    for name in (a.only or []) + ([a.profile] if a.profile else []):
        if name not in calls:
            ap.error(f"--family {a.family} has the passes {', '.join(calls)}, not {name!r}")
    if a.profile:
        calls[a.profile]()
        return

    def timed(fn):
        fn()  # warm: handle, plans, tables
        ts = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return [round(1e3 * t / a.ntimes, 3) for t in ts]

    out = dict(head, nsrc=int(np.size(cfg["ra"])), nbls=len(cfg["baselines"]), nfreq=a.nfreq, ntimes=a.ntimes)
    for name, fn in calls.items():
        if a.only and name not in a.only:
            continue
        runs = timed(fn)
        out[name + "_ms_per_step"] = round(float(np.median(runs)), 3)
        if spread == "runs":
            out[name + "_runs"] = runs
        elif spread == "range":
            out[name + "_range"] = [min(runs), max(runs)]
        print(json.dumps({name: runs}), file=sys.stderr, flush=True)
    for key, (num, den) in ratios.items():
        num, den = (num,) if isinstance(num, str) else num, (den,) if isinstance(den, str) else den
        if all(k + "_ms_per_step" in out for k in num + den):
            out[key] = round(sum(out[k + "_ms_per_step"] for k in num) / sum(out[k + "_ms_per_step"] for k in den), 3)
    if all(k + "_ms_per_step" in out for k in ("forward", "tangent_1", "tangent_n")):  # (basis_tangent)
        # per direction, against TWO forward runs: what (V(C + D) - V(C - D)) / 2 costs a caller without the pass
        two = 2.0 * out["forward_ms_per_step"]
        out["tangent_1_over_two_forwards"] = round(out["tangent_1_ms_per_step"] / two, 3)
        out["tangent_n_per_direction_over_two_forwards"] = round(out["tangent_n_ms_per_step"] / a.ndir / two, 3)
        out["further_direction_ms_per_step"] = round((out["tangent_n_ms_per_step"] - out["tangent_1_ms_per_step"]) /
                                                     max(a.ndir - 1, 1), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
