"""Basis beams, positions: forward vs the position adjoint and the position tangent through basis beams, time per time
step, on one configuration.

    python tools/basis_position_timing.py [--config C5] [--nsrc N] [--nfreq 8] [--ntimes 2] [--repeats 3]
    python tools/basis_position_timing.py --forward-only   (runs on a commit without the passes: the parent's forward)

Prints one JSON line: ms per time step of simulate_vis, of simulate_vis_basis_adjoint(wrt="baselines") and of
simulate_vis_basis_jvp(d_baselines=) (wall clock of a whole call on a warm handle, divided by the time steps; the median
of --repeats calls, with the values), and each pass as a ratio to the forward of the same run.  The ratio to the parent
commit's forward is taken from a --forward-only run of the parent's tree in the same job.
--profile PASS: one call of that pass on a cold handle and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/basis_position_timing.py --profile adjoint)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fftvis_amd  # noqa: E402
from fftvis_amd import synth  # noqa: E402

PASSES = ["forward", "adjoint", "tangent"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--nsrc", type=int, default=None)
    ap.add_argument("--nfreq", type=int, default=8)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--profile", choices=PASSES, default=None)
    a = ap.parse_args()
    cfg = synth.make_config(a.config, nsrc=a.nsrc, nfreq=a.nfreq, ntimes=a.ntimes)
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    nbls = len(cfg["baselines"])
    cdt = np.complex64 if cfg["precision"] == 1 else np.complex128
    rng = np.random.default_rng(0)
    g = (rng.normal(size=(a.nfreq, a.ntimes, 2, 2, nbls)) + 0j).astype(cdt)
    db = rng.normal(size=(nbls, 3))
    calls = {"forward": lambda: fftvis_amd.simulate_vis(**cfg)}
    if not a.forward_only:
        calls["adjoint"] = lambda: fftvis_amd.simulate_vis_basis_adjoint(g, **cfg, wrt="baselines")
        calls["tangent"] = lambda: fftvis_amd.simulate_vis_basis_jvp(**cfg, d_baselines=db)
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
           "nbasis": len(cfg["beam"]), "precision": cfg["precision"]}
    for name, fn in calls.items():
        out[name + "_ms_per_step"], out[name + "_runs"] = timed(fn)
        print(json.dumps({name: out[name + "_runs"]}), file=sys.stderr, flush=True)
    for name in ("adjoint", "tangent"):
        if name + "_ms_per_step" in out:
            out[name + "_over_forward"] = round(out[name + "_ms_per_step"] / out["forward_ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
