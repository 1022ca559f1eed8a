"""Source positions: forward, flux adjoint and source pass, time per time step, on HERA-350 with C3's catalog, beam and band.

    python tools/source_adjoint_timing.py                  (forward, simulate_vis_adjoint, simulate_vis_source_adjoint)
    python tools/source_adjoint_timing.py --without-sources   (runs on a commit without the gradient: the parent's two)

Prints one JSON line: ms per time step of each call (wall clock of a whole call on a warm handle, divided by the time
steps; the median of --repeats calls) and the source pass's ratios to the other two.
--profile PASS: one call of that pass on a cold handle and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/source_adjoint_timing.py --profile sources)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fftvis_amd  # noqa: E402
from fftvis_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsrc", type=int, default=None)
    ap.add_argument("--nfreq", type=int, default=8)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--without-sources", action="store_true")
    ap.add_argument("--profile", choices=["forward", "fluxes", "sources"], default=None)
    a = ap.parse_args()
    cfg = synth.make_config("C3", nsrc=a.nsrc, nfreq=a.nfreq, ntimes=a.ntimes)
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    nbls = len(cfg["baselines"])
    shape = (a.nfreq, a.ntimes, 2, 2, nbls) if cfg["polarized"] else (a.nfreq, a.ntimes, nbls)
    g = np.random.default_rng(0).normal(size=shape) + 0j
    no_flux = {k: v for k, v in cfg.items() if k != "fluxes"}
    calls = {"forward": lambda: fftvis_amd.simulate_vis(**cfg),
             "fluxes": lambda: fftvis_amd.simulate_vis_adjoint(g, **no_flux, full_stokes=np.ndim(cfg["fluxes"]) == 3)}
    if not a.without_sources:
        calls["sources"] = lambda: fftvis_amd.simulate_vis_source_adjoint(g, **cfg, wrt="radec")
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

    out = {"nsrc": int(np.size(cfg["ra"])), "nbls": nbls, "nfreq": a.nfreq, "ntimes": a.ntimes, "precision": cfg["precision"],
           "polarized": bool(cfg["polarized"])}
    for name, fn in calls.items():
        out[name + "_ms_per_step"], out[name + "_runs"] = timed(fn)
    if "sources" in calls:
        out["sources_over_fluxes"] = round(out["sources_ms_per_step"] / out["fluxes_ms_per_step"], 3)
        out["sources_over_forward"] = round(out["sources_ms_per_step"] / out["forward_ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
