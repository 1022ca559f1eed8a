"""Basis beams: forward vs flux pass vs coefficient pass, time per time step, on one configuration.

    python tools/basis_adjoint_timing.py --config C5 [--nsrc N] [--nfreq 4] [--ntimes 2] [--repeats 3]
    python tools/basis_adjoint_timing.py --small          (HERA-37, K = 3 Airy dishes, fp64)
    python tools/basis_adjoint_timing.py --forward-only   (runs on a commit without the gradients: the parent's forward)

Prints one JSON line: ms per time step of simulate_vis and of simulate_vis_basis_adjoint with wrt = fluxes, beam_coefs
and both (wall clock of a whole call on a warm handle, divided by the time steps; the median of --repeats calls).
--profile PASS: one call of that pass on a cold handle and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/basis_adjoint_timing.py --profile beam_coefs)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fftvis_amd  # noqa: E402
from fftvis_amd import synth  # noqa: E402


def small_config(nfreq, ntimes):
    """HERA-37 (C2's array), 1e4 sources, three Airy dishes as basis beams, random coefficients, fp64, eps 6e-8."""
    cfg = synth.make_config("C2", nfreq=nfreq, ntimes=ntimes)
    rng = np.random.default_rng(1)
    nant = len(cfg["ants"])
    coefs = 0.05 * (rng.normal(size=(nant, 3, nfreq)) + 1j * rng.normal(size=(nant, 3, nfreq)))
    coefs[:, 0, :] += 1.0
    cfg.update(polarized=True, beam=[fftvis_amd.AiryBeam(d) for d in (14.0, 13.0, 15.0)], beam_coefs=coefs)
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--nsrc", type=int, default=None)
    ap.add_argument("--nfreq", type=int, default=4)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--profile", choices=["forward", "fluxes", "beam_coefs"], default=None)
    a = ap.parse_args()
    cfg = small_config(a.nfreq, a.ntimes) if a.small else synth.make_config(a.config, nsrc=a.nsrc, nfreq=a.nfreq,
                                                                           ntimes=a.ntimes)
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    nbls = len(cfg["baselines"])
    cdt = np.complex64 if cfg["precision"] == 1 else np.complex128
    g = (np.random.default_rng(0).normal(size=(a.nfreq, a.ntimes, 2, 2, nbls)) + 0j).astype(cdt)
    calls = {"forward": lambda: fftvis_amd.simulate_vis(**cfg)}
    if not a.forward_only:
        for name, wrt in (("fluxes", "fluxes"), ("beam_coefs", "beam_coefs"), ("both", ("fluxes", "beam_coefs"))):
            calls[name] = lambda wrt=wrt: fftvis_amd.simulate_vis_basis_adjoint(g, **cfg, wrt=wrt)
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
        return round(1e3 * float(np.median(ts)) / a.ntimes, 3)

    out = {"config": "small" if a.small else a.config, "nsrc": int(np.size(cfg["ra"])), "nbls": nbls, "nfreq": a.nfreq,
           "ntimes": a.ntimes, "nbasis": len(cfg["beam"]), "precision": cfg["precision"]}
    for name, fn in calls.items():
        out[name + "_ms_per_step"] = timed(fn)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
