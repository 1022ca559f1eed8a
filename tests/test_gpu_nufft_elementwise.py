"""The type-3 transform op (``gpu_nufft2d`` / ``gpu_nufft3d``) and the device's brute-force checker (``gpu_nudft_direct``)
element by element against the extended-precision exact sum, on seeded cases that put targets and sources on the corners
and edges of their boxes, give the rows of ``c`` scales from 1e-6 to 1e6, walk the anisotropic and tiny grids, force every
spread scheme and both treatments of the third dimension, and degenerate in every way the op accepts.

Every comparison is ``tests.nufft_op_refs.check``: per (transform, target) ``|got - exact| / (eps ||c_t||_2)`` against
``2 max(Y_case, Y_plain) + floor`` and per row its rel l2 against ``max(5 eps, 2 port's) + floor`` -- the Y's are the CPU
port's own worst elements on the same case and on the family's plain case, never the device's.  fp32 runs are judged against
the exact sum of the inputs rounded to float32.  FFTVIS_TEST_METRICS=<file> logs one JSON line per comparison."""

import json
import os

import numpy as np
import pytest

from fftvis_amd import _lib
from fftvis_amd.gpu import gpu_nufft2d, gpu_nufft3d
from fftvis_amd.gpu.nufft import gpu_nudft_direct
from tests import nufft_op_refs as R

pytestmark = pytest.mark.gpu

SPREAD_PATHS = {"matrix product": {"FFTVIS_HIP_SPREAD_MM": "1"},
                "lane per (cell, channel group)": {"FFTVIS_HIP_SPREAD_MM": "0", "FFTVIS_HIP_SPREAD_CELL": "0"},
                "lane per cell": {"FFTVIS_HIP_SPREAD_MM": "0", "FFTVIS_HIP_SPREAD_CELL": "1"}}
Z_PATHS = {"direct z": None, "three passes": "1"}


def _device(name, eps, sigma):
    cs = R.case(name)
    fn = gpu_nufft2d if cs["dim"] == 2 else gpu_nufft3d
    out = fn(*cs["coords"], cs["c"], *cs["targets"], eps, upsample_factor=sigma)
    assert out.dtype == (np.complex64 if cs["precision"] == 1 else np.complex128) and out.shape == R.exact(name)[0].shape
    return out


@pytest.fixture
def z_path(request, monkeypatch):
    """The treatment of the third dimension is read when the plan is built and the plan is cached per thread: release
    the workspaces on either side of the switch."""
    _lib.lib().fv_release_workspaces()
    if Z_PATHS[request.param] is None:
        monkeypatch.delenv("FFTVIS_HIP_NO_ZDIRECT", raising=False)
    else:
        monkeypatch.setenv("FFTVIS_HIP_NO_ZDIRECT", Z_PATHS[request.param])
    yield request.param
    _lib.lib().fv_release_workspaces()


@pytest.mark.parametrize("name,eps,sigma", R.combos(R.CASES_FP64_2D))
def test_nufft2d_fp64(gpu, name, eps, sigma):
    R.check(_device(name, eps, sigma), name, eps, sigma, path="default")


@pytest.mark.parametrize("path", list(SPREAD_PATHS))
@pytest.mark.parametrize("name", ["2d_rowscales_5", "2d_rowscales_19", "2d_rowscales_24"])
def test_nufft2d_row_scales_on_every_spread_scheme(gpu, monkeypatch, name, path):
    """Rows of c from 1e-6 to 1e6 with 150 sources in one bin, 5 / 19 / 24 transforms (chunks of 16, 8 and fewer) on each
    forced accumulation scheme: a row must not feel its neighbours.  Then the same rows permuted: every result follows
    its row."""
    for k, v in SPREAD_PATHS[path].items():
        monkeypatch.setenv(k, v)
    for _, eps, sigma in R.combos([name]):
        R.check(_device(name, eps, sigma), name, eps, sigma, path=path)
    cs = R.case(name)
    perm = np.random.default_rng(7).permutation(cs["c"].shape[0])
    for eps, sigma in ((1e-9, 2.0), (1e-6, 1.25)):
        got = gpu_nufft2d(*cs["coords"], np.ascontiguousarray(cs["c"][perm]), *cs["targets"], eps, upsample_factor=sigma)
        R.check(got, name, eps, sigma, rows=perm, path=path, label="rows permuted")


@pytest.mark.parametrize("z_path", list(Z_PATHS), indirect=True)
@pytest.mark.parametrize("name,eps,sigma", R.combos(R.CASES_FP64_3D))
def test_nufft3d_fp64(gpu, z_path, name, eps, sigma):
    R.check(_device(name, eps, sigma), name, eps, sigma, path=z_path)


@pytest.mark.parametrize("name,eps,sigma", R.combos([n for n in R.CASES_FP32 if n.startswith("2d")]))
def test_nufft2d_fp32(gpu, name, eps, sigma):
    R.check(_device(name, eps, sigma), name, eps, sigma, path="default")


@pytest.mark.parametrize("z_path", list(Z_PATHS), indirect=True)
@pytest.mark.parametrize("name,eps,sigma", R.combos([n for n in R.CASES_FP32 if n.startswith("3d")]))
def test_nufft3d_fp32(gpu, z_path, name, eps, sigma):
    R.check(_device(name, eps, sigma), name, eps, sigma, path=z_path)


@pytest.mark.parametrize("name", ["2d_corners", "2d_offcentre", "2d_rowscales_19", "2d_coincident", "3d_cubic",
                                  "2d_corners32", "3d_corners32"])
def test_nudft_direct_is_an_exact_sum(gpu, name):
    """The device's checker is held as what it is: no multiple of any eps, only the rounding of its own phases (term 1 of
    ``floor``) and of adding M terms, M u ||c_t||_2, at the precision of its inputs."""
    cs = R.case(name)
    got = gpu_nudft_direct(cs["coords"], cs["c"], cs["targets"])
    assert got.dtype == cs["c"].dtype
    err = R._err(got, R.exact(name))
    M = cs["c"].shape[1]
    lim = R.phase_term(cs) + M * R.unit_roundoff(cs["precision"]) * R.row_norms(cs["c"])[1]
    worst = float((err / lim[:, None]).max())
    if os.environ.get("FFTVIS_TEST_METRICS"):
        with open(os.environ["FFTVIS_TEST_METRICS"], "a") as f:
            f.write(json.dumps({"case": name, "path": "gpu_nudft_direct", "precision": cs["precision"],
                                "worst_over_limit": worst, "test": os.environ.get("PYTEST_CURRENT_TEST", "")}) + "\n")
    assert np.isfinite(err).all() and worst <= 1.0, (name, worst)


@pytest.mark.parametrize("name,sigma,eps", R.SENSITIVITY)
def test_device_at_100_eps_is_rejected(gpu, name, sigma, eps):
    """The check has teeth on the device's own output: the transform run 100 times too coarse fails both assertions."""
    m = R.judge(_device(name, 100 * eps, sigma), name, eps, sigma, path="default", label="run at 100 eps")
    assert not m["ok_element"] and not m["ok_rows"], m
