"""Forward vs adjoint time per time step (simulate_vis / simulate_vis_adjoint) on one configuration.

    python tools/adjoint_timing.py --config C3 [--nfreq 2] [--ntimes 2] [--repeats 3] [--lattice]
                                   [--adjoint-path type3|type2|auto] [--package DIR]

Prints one JSON line: ms per time step of each (wall clock of a whole call on a warm handle, divided by the time
steps; the median of --repeats calls, and their spread).  --lattice: the reference's default call on a griddable array
(force_use_type3=False: the forward is the type-1 transform); --adjoint-path: the adjoint's transform there.  --package:
the checkout whose fftvis_amd is measured (an earlier commit's, built in place: this script runs against it unchanged as
long as --adjoint-path is type3).  tools/adjoint_timing.sh runs it for C2 and C3 and a kernel-trace profile."""

import argparse
import json
import os
import sys
import time

import numpy as np



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--nfreq", type=int, default=2)
    ap.add_argument("--ntimes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--adjoint-only", action="store_true", help="(profiling) one adjoint call on a cold handle, no forward run")
    ap.add_argument("--lattice", action="store_true", help="force_use_type3=False: the type-1 forward on a griddable array")
    ap.add_argument("--adjoint-path", default="type3", choices=["type3", "type2", "auto"])
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose fftvis_amd is measured (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import fftvis_amd
    from fftvis_amd import synth

    cfg = synth.make_config(a.config, nfreq=a.nfreq, ntimes=a.ntimes)
    cfg["upsample_factor"] = "auto"  # the benchmark's setting
    if a.lattice:
        cfg["force_use_type3"] = False
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    if a.adjoint_path != "type3":  # (the default is left out: a checkout from before the keyword takes the same call)
        kw["adjoint_path"] = a.adjoint_path
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
        ms = 1e3 * np.array(ts) / a.ntimes
        return float(np.median(ms)), [round(float(ms.min()), 3), round(float(ms.max()), 3)]

    fwd, fwd_range = timed(lambda: fftvis_amd.simulate_vis(**cfg))
    adj, adj_range = timed(lambda: fftvis_amd.simulate_vis_adjoint(g, **kw))
    print(json.dumps({"config": a.config, "nsrc": int(np.size(cfg["ra"])), "nbls": len(cfg["baselines"]),
                      "nfreq": a.nfreq, "ntimes": a.ntimes, "polarized": bool(cfg["polarized"]),
                      "lattice": bool(a.lattice), "adjoint_path": a.adjoint_path,
                      "forward_ms_per_step": round(fwd, 3), "forward_range": fwd_range,
                      "adjoint_ms_per_step": round(adj, 3), "adjoint_range": adj_range,
                      "adjoint_over_forward": round(adj / fwd, 3)}))


if __name__ == "__main__":
    main()
