"""Worker of tests/test_gpu_fft_stage.py: every combination of ``tests.fft_stage_refs.COMBOS`` through ``gpu_nufft2d`` in
one process, under whatever FFTVIS_HIP_* switches the parent set (they are read once per process), saved as one ``.npz``:
``r<i>`` the result of combination i, ``refused`` the indices the library refused with an argument error (``FV_REQUIRE``:
nothing was launched) and why.  Before each call a marker line goes to stderr, so that the parent can tell which call the
``rowfft ...`` lines of FFTVIS_HIP_DEBUG_FFT belong to.  Any other error ends the worker at once with a non-zero status.

usage: python tests/fft_stage_worker.py OUT.npz"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fftvis_amd import _lib  # noqa: E402
from fftvis_amd.gpu import gpu_nufft2d  # noqa: E402
from tests import fft_stage_refs as F  # noqa: E402
from tests import nufft_op_refs as R  # noqa: E402

MARK = "fft_stage_worker call "


def run(name, eps, sigma):
    cs = R.case(name)
    return gpu_nufft2d(*cs["coords"], cs["c"], *cs["targets"], eps, upsample_factor=sigma)


if __name__ == "__main__":
    out, refused = {}, {}
    for i, (name, eps, sigma) in enumerate(F.COMBOS):
        print(f"{MARK}{i} {name} {eps:g} {sigma:g}", file=sys.stderr, flush=True)
        try:
            out[f"r{i}"] = run(name, eps, sigma)
        except _lib.FftvisHipError as e:
            if not str(e).startswith("libfftvis_hip status 1:"):  # anything but a refused argument: stop here
                raise
            refused[str(i)] = str(e)
    np.savez(sys.argv[1], refused=np.array(json.dumps(refused)), **out)
