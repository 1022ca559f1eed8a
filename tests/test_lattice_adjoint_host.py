"""CPU tests of the lattice path's type-2 adjoint (``adjoint_path=``): the C entry points and their argument checks, the
keyword's validation before any device work, what ``torch_simulate_vis`` hands to ``simulate_vis``, and the oracle's two
forms of the exact transpose on a lattice."""

import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from tests.helpers import oracle_adjoint, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fv_sim_set_adjoint_path", "fv_sim_last_adjoint_path")


def _cfg(**kw):
    c = synth.make_config("C1", nsrc=20, nfreq=3, ntimes=2)
    return dict({k: v for k, v in c.items() if k != "fluxes"}, **kw)


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fftvis_hip.h")).read()
    declared = set(re.findall(r"^int\s*(fv_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    # each answers to reference lines, as every entry point of the header does
    doc = hdr[hdr.index("/* Which transform fv_sim_run_adjoint uses"):hdr.index("int fv_sim_last_adjoint_path")]
    assert "cpu_simulate.py:" in doc and "nufft.py:" in doc


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    assert L.fv_sim_set_adjoint_path(None, 1) == 1
    assert b"handle" in L.fv_last_error()
    assert L.fv_sim_last_adjoint_path(None) == 1  # FV_ERR_ARG: not one of the paths 0, 2, 3
    assert b"handle" in L.fv_last_error()


@pytest.mark.parametrize("bad", ["nonsense", "type1", "", None, 2])
def test_unknown_adjoint_path_raises_before_device_work(bad):
    cfg = _cfg()
    with pytest.raises(ValueError, match="adjoint_path"):
        fftvis_amd.simulate_vis_adjoint(np.zeros((3, 2, 21), complex), **cfg, adjoint_path=bad)
    with pytest.raises(ValueError, match="adjoint_path"):
        fftvis_amd.torch_simulate_vis(None, **cfg, adjoint_path=bad)


def test_known_adjoint_paths():
    from fftvis_amd.gpu import gpu_simulate

    assert gpu_simulate.ADJOINT_PATHS == ("type3", "type2", "auto")
    import inspect

    assert inspect.signature(fftvis_amd.simulate_vis_adjoint).parameters["adjoint_path"].default == "type3"
    assert inspect.signature(gpu_simulate.GPUSimulationEngine.simulate).parameters["adjoint_path"].default == "type3"
    assert "adjoint_path" not in inspect.signature(fftvis_amd.simulate_vis_basis_adjoint).parameters


def test_torch_simulate_vis_keeps_adjoint_path_from_the_forward(monkeypatch):
    """The keyword goes to the backward pass only: ``simulate_vis`` never sees it, ``simulate_vis_adjoint`` does."""
    import torch

    from fftvis_amd import adjoint, wrapper

    cfg = _cfg()
    seen = {}

    def fake_forward(**kw):
        seen["forward"] = set(kw)
        return np.zeros((3, 2, 21), complex)

    def fake_adjoint(g, **kw):
        seen["backward"] = kw.get("adjoint_path")
        return np.ones((20, 3))

    monkeypatch.setattr(wrapper, "simulate_vis", fake_forward)
    monkeypatch.setattr(adjoint, "simulate_vis_adjoint", fake_adjoint)
    F = torch.ones((20, 3), dtype=torch.float64, requires_grad=True)
    V = fftvis_amd.torch_simulate_vis(F, adjoint_path="type2", **cfg)
    assert "adjoint_path" not in seen["forward"] and {"fluxes", "ants", "freqs"} <= seen["forward"]
    V.abs().sum().backward()
    assert seen["backward"] == "type2"
    assert F.grad is not None and F.grad.shape == F.shape


@pytest.mark.parametrize("polarized,full", [(False, False), (True, True)])
def test_oracle_transposes_agree_on_a_lattice(polarized, full):
    """The oracle's exact transpose through the lattice form (integer modes) and through the baseline vectors: the same
    map, to rounding."""
    cfg = dict(synth.make_config("C1", nsrc=25, nfreq=3, ntimes=2), polarized=polarized)
    cfg["baselines"] = cfg["baselines"] + [(3, 0), (6, 1), (2, 2)]
    nbl = len(cfg["baselines"])
    rng = np.random.default_rng(3)
    shape = (3, 2, 2, 2, nbl) if polarized else (3, 2, nbl)
    G = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    lattice = oracle_adjoint(dict(cfg, force_use_type3=False), G, full_stokes=full)
    vectors = oracle_adjoint(dict(cfg, force_use_type3=True), G, full_stokes=full)
    assert np.count_nonzero(lattice) > 0
    assert rel_l2(lattice, vectors) <= 1e-12
