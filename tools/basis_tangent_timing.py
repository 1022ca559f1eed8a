"""Basis beams, forward mode: forward vs the coefficient tangent with 1 and with 8 directions vs the coefficient-gradient
pass, time per time step, on one configuration.

    python tools/basis_tangent_timing.py [--config C5] [--nsrc N] [--nfreq 8] [--ntimes 2] [--repeats 3] [--ndir 8]

Prints one JSON line: ms per time step of simulate_vis, of simulate_vis_basis_jvp with one direction and with --ndir
directions of the coefficients, and of simulate_vis_basis_adjoint(wrt="beam_coefs") (wall clock of a whole call on a warm
handle, divided by the time steps; the median of --repeats calls, with the values), and the tangents' cost per direction
as a ratio to TWO forward runs -- what (V(C + D) - V(C - D)) / 2 costs a caller without the pass.
--profile PASS: one call of that pass on a cold handle and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/basis_tangent_timing.py --profile tangent_n)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fftvis_amd  # noqa: E402
from fftvis_amd import synth  # noqa: E402

PASSES = ["forward", "tangent_1", "tangent_n", "beam_coefs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--nsrc", type=int, default=None)
    ap.add_argument("--nfreq", type=int, default=8)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ndir", type=int, default=8)
    ap.add_argument("--only", choices=PASSES, action="append", default=None)
    ap.add_argument("--profile", choices=PASSES, default=None)
    a = ap.parse_args()
    cfg = synth.make_config(a.config, nsrc=a.nsrc, nfreq=a.nfreq, ntimes=a.ntimes)
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    nbls = len(cfg["baselines"])
    cdt = np.complex64 if cfg["precision"] == 1 else np.complex128
    rng = np.random.default_rng(0)
    g = (rng.normal(size=(a.nfreq, a.ntimes, 2, 2, nbls)) + 0j).astype(cdt)
    shape = np.shape(cfg["beam_coefs"])
    d = (rng.normal(size=(a.ndir,) + shape) + 1j * rng.normal(size=(a.ndir,) + shape)).astype(cdt)
    calls = {"forward": lambda: fftvis_amd.simulate_vis(**cfg),
             "tangent_1": lambda: fftvis_amd.simulate_vis_basis_jvp(**cfg, d_beam_coefs=d[0]),
             "tangent_n": lambda: fftvis_amd.simulate_vis_basis_jvp(**cfg, d_beam_coefs=d),
             "beam_coefs": lambda: fftvis_amd.simulate_vis_basis_adjoint(g, **cfg, wrt="beam_coefs")}
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
        return round(1e3 * float(np.median(ts)) / a.ntimes, 3), [round(1e3 * t / a.ntimes, 3) for t in ts]

    out = {"config": a.config, "nsrc": int(np.size(cfg["ra"])), "nbls": nbls, "nfreq": a.nfreq, "ntimes": a.ntimes,
           "nbasis": len(cfg["beam"]), "precision": cfg["precision"], "ndir": a.ndir}
    for name, fn in calls.items():
        if a.only and name not in a.only:
            continue
        out[name + "_ms_per_step"], out[name + "_runs"] = timed(fn)
        print(json.dumps({name: out[name + "_runs"]}), file=sys.stderr, flush=True)
    if all(k + "_ms_per_step" in out for k in ("forward", "tangent_1", "tangent_n")):
        two = 2.0 * out["forward_ms_per_step"]
        out["tangent_1_over_two_forwards"] = round(out["tangent_1_ms_per_step"] / two, 3)
        out["tangent_n_per_direction_over_two_forwards"] = round(out["tangent_n_ms_per_step"] / a.ndir / two, 3)
        out["further_direction_ms_per_step"] = round((out["tangent_n_ms_per_step"] - out["tangent_1_ms_per_step"]) /
                                                     max(a.ndir - 1, 1), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
