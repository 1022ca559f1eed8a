"""Tangents: forward, the two position adjoints and the three tangents, time per time step, on HERA-350 with C3's
catalog, beam and band.

    python tools/tangent_timing.py --array ideal      (coplanar, redundant)
    python tools/tangent_timing.py --array surveyed   (seeded N(0, 2 cm) errors in x, y and 3 cm in z)
    python tools/tangent_timing.py --parent           (runs on a commit without the tangent -- or on its library through
                                                       FFTVIS_HIP_LIB: forward, position pass and source pass only)

Prints one JSON line: ms per time step of each call (wall clock of a whole call on a warm handle, divided by the time
steps; the median of --repeats calls, with the values).
--profile PASS: one call of that pass on a cold handle and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/tangent_timing.py --profile tangent_baselines)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fftvis_amd  # noqa: E402
from fftvis_amd import synth  # noqa: E402

PASSES = ["forward", "position", "source", "tangent_baselines", "tangent_directions", "tangent_both"]


def surveyed(ants, seed=2):
    """The array with seeded survey errors: N(0, 2 cm) in x and y, N(0, 3 cm) in z."""
    rng = np.random.default_rng(seed)
    err = rng.normal(size=(len(ants), 3)) * np.array([0.02, 0.02, 0.03])
    return {k: np.asarray(p, float) + err[i] for i, (k, p) in enumerate(ants.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--array", choices=["ideal", "surveyed"], default="ideal")
    ap.add_argument("--nsrc", type=int, default=None)
    ap.add_argument("--nfreq", type=int, default=8)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--only", choices=PASSES, action="append", default=None)
    ap.add_argument("--profile", choices=PASSES, default=None)
    a = ap.parse_args()
    cfg = synth.make_config("C3", nsrc=a.nsrc, nfreq=a.nfreq, ntimes=a.ntimes)
    if a.array == "surveyed":
        cfg["ants"] = surveyed(cfg["ants"])
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    nbls, nsrc = len(cfg["baselines"]), int(np.size(cfg["ra"]))
    rng = np.random.default_rng(0)
    g = rng.normal(size=(a.nfreq, a.ntimes, 2, 2, nbls)) + 0j
    db, dt = rng.normal(size=(nbls, 3)), rng.normal(size=(a.ntimes, nsrc, 3))
    calls = {"forward": lambda: fftvis_amd.simulate_vis(**cfg),
             "position": lambda: fftvis_amd.simulate_vis_position_adjoint(g, **cfg, wrt="baselines"),
             "source": lambda: fftvis_amd.simulate_vis_source_adjoint(g, **cfg, wrt="topo")}
    if not a.parent:
        calls["tangent_baselines"] = lambda: fftvis_amd.simulate_vis_jvp(**cfg, d_baselines=db)
        calls["tangent_directions"] = lambda: fftvis_amd.simulate_vis_jvp(**cfg, d_topo=dt)
        calls["tangent_both"] = lambda: fftvis_amd.simulate_vis_jvp(**cfg, d_baselines=db, d_topo=dt)
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

    out = {"array": a.array, "nsrc": nsrc, "nbls": nbls, "nfreq": a.nfreq, "ntimes": a.ntimes, "precision": cfg["precision"],
           "lib": os.environ.get("FFTVIS_HIP_LIB", "in-tree")}
    for name, fn in calls.items():
        if a.only and name not in a.only:
            continue
        out[name + "_ms_per_step"], out[name + "_runs"] = timed(fn)
        print(json.dumps({name: out[name + "_runs"]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
