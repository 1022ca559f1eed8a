"""Forward vs adjoint time per time step (simulate_vis / simulate_vis_adjoint) on one configuration.

    python tools/adjoint_timing.py --config C3 [--nfreq 2] [--ntimes 2] [--repeats 3]

Prints one JSON line: ms per time step of each (wall clock of a whole call on a warm handle, divided by the time
steps; the median of --repeats calls).  tools/adjoint_timing.sh runs it for C2 and C3 and a kernel-trace profile."""

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
    ap.add_argument("--config", default="C3")
    ap.add_argument("--nfreq", type=int, default=2)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--adjoint-only", action="store_true", help="(profiling) one adjoint call on a cold handle, no forward run")
    a = ap.parse_args()
    cfg = synth.make_config(a.config, nfreq=a.nfreq, ntimes=a.ntimes)
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    nbls = len(cfg["baselines"])
    shape = (a.nfreq, a.ntimes, 2, 2, nbls) if cfg["polarized"] else (a.nfreq, a.ntimes, nbls)
    g = np.random.default_rng(0).normal(size=shape) + 0j
    if a.adjoint_only:
        fftvis_amd.simulate_vis_adjoint(g, **kw)
        return

    def timed(fn):
        fn()  # warm: handle, plans, tables
        ts = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return 1e3 * float(np.median(ts)) / a.ntimes

    fwd = timed(lambda: fftvis_amd.simulate_vis(**cfg))
    adj = timed(lambda: fftvis_amd.simulate_vis_adjoint(g, **kw))
    print(json.dumps({"config": a.config, "nsrc": int(np.size(cfg["ra"])), "nbls": len(cfg["baselines"]),
                      "nfreq": a.nfreq, "ntimes": a.ntimes, "polarized": bool(cfg["polarized"]),
                      "forward_ms_per_step": round(fwd, 3), "adjoint_ms_per_step": round(adj, 3),
                      "adjoint_over_forward": round(adj / fwd, 3)}))


if __name__ == "__main__":
    main()
