"""The pruned FFT stage (``k_rowfft_st`` / ``k_rowfft_dif``) held to FFT rounding, on every slot of every plan of the
ladder in tests/fft_stage_refs.py: cases dense in one long dimension, so that every input slot carries a number and every
output index is read.

* The plan each run launches is read from ``FFTVIS_HIP_DEBUG_FFT=1`` and must be the host model's; the union over the
  module must contain the whole table (a folded Q = 4096 row pass and a folded ``k_rowfft_dif`` pass among it).
* Anchor: every result against the extended-precision exact sum, ``nufft_op_refs.check`` unchanged.
* Differential: the same runs in child processes under FFTVIS_HIP_OLD_FFT=1 (every pass on ``k_rowfft_dif``, a second
  independent FFT), FFTVIS_HIP_PAIR=0 / 2 and FFTVIS_HIP_NATURAL_ORDER=1.  Spread, deconvolution and gather are the same
  deterministic kernels in all of them, so a difference is the FFT's alone and is held per (transform, target) to
  ``K u (sum_d log2 n2_d) A_k ||c_t||_2`` with ``K = 4 max(Z_case, 1)`` from the CPU port (fft_stage_refs.z_case).

FFTVIS_TEST_METRICS=<file> logs one JSON line per comparison."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fftvis_amd import _lib
from fftvis_amd.gpu import gpu_nufft2d
from tests import fft_stage_refs as F
from tests import nufft_op_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = sorted({k for env in F.REALISATIONS.values() for k in env})
_DEFAULT = {}  # (name, eps, sigma) -> (result, passes the debug line reported)


def _id(combo):
    return f"{combo[0]}-{combo[1]:g}-{combo[2]:g}"


def _log(rec):
    if os.environ.get("FFTVIS_TEST_METRICS"):
        with open(os.environ["FFTVIS_TEST_METRICS"], "a") as f:
            f.write(json.dumps(dict(rec, test=os.environ.get("PYTEST_CURRENT_TEST", ""))) + "\n")


def _default(combo, capfd, monkeypatch):
    """The combination on the default kernels, in this process, with the passes it reported (run once per module)."""
    if combo not in _DEFAULT:
        assert not [k for k in SWITCHES if k in os.environ], "the default realisation needs the FFT switches unset"
        name, eps, sigma = combo
        cs = R.case(name)
        monkeypatch.setenv("FFTVIS_HIP_DEBUG_FFT", "1")
        capfd.readouterr()
        try:
            out = gpu_nufft2d(*cs["coords"], cs["c"], *cs["targets"], eps, upsample_factor=sigma)
        except _lib.FftvisHipError as e:
            if not str(e).startswith("libfftvis_hip status 1:"):  # a HIP error: nothing more is started on this device
                pytest.exit(f"{combo}: {e}", returncode=3)
            raise
        passes = F.parse_debug(capfd.readouterr().err)
        monkeypatch.delenv("FFTVIS_HIP_DEBUG_FFT")
        assert out.dtype == (np.complex64 if cs["precision"] == 1 else np.complex128)
        assert out.shape == cs["c"].shape[:1] + cs["targets"][0].shape
        out.setflags(write=False)
        _DEFAULT[combo] = (out, passes)
    return _DEFAULT[combo]


def _same_plan(passes, name, eps, sigma, pair=(0, 0)):
    """The two passes a run reported against the host model: lengths, factorisation, fold and pairing."""
    assert len(passes) == 2, passes
    for got, want, pr in zip(passes, F.plan(name, eps, sigma), pair):
        for k in ("col", "n_in", "n_out", "n2", "P", "Q", "folded"):
            assert got[k] == want[k], (name, eps, sigma, k, got, want)
        assert got["pair"] == pr, (name, eps, sigma, got)


@pytest.mark.parametrize("combo", F.COMBOS, ids=_id)
def test_launched_plan_is_the_modelled_one(gpu, capfd, monkeypatch, combo):
    name, eps, sigma = combo
    passes = _default(combo, capfd, monkeypatch)[1]
    _same_plan(passes, name, eps, sigma)
    want = F.table_entry(name, eps, sigma)
    if want is not None:  # the rung is a line of the table: that very plan, in the long dimension
        g = passes[R.case(name)["long_dim"]]
        assert (g["P"], g["Q"], g["folded"]) == want, (name, eps, sigma, g, want)
    _log({"case": name, "eps": eps, "sigma": sigma, "path": "plan",
          "passes": [[g["col"], g["n_in"], g["n_out"], g["P"], g["Q"], g["rpw"], g["pair"]] for g in passes]})


def test_ladder_launches_every_plan_of_the_table(gpu, capfd, monkeypatch):
    seen, seen32 = set(), set()
    for combo in F.COMBOS:
        for g in _default(combo, capfd, monkeypatch)[1]:
            (seen32 if combo[0] in F.CASES_FP32 else seen).add((g["col"], g["P"], g["Q"], g["folded"]))
    missing = F.expected_table() - seen
    assert not missing, sorted(missing)
    assert (0, 4, 4096, True) in seen and (0, 3, 4096, True) in seen  # a folded Q = 4096 row pass
    assert {(0, 5, 64, True), (0, 5, 128, True), (0, 5, 256, True)} <= seen  # folded k_rowfft_dif passes
    assert {(0,) + v for v in F.FP32_TABLE.values()} <= seen32
    # the blocked family: both passes on the register-resident kernels, either orientation, folded and not
    assert {(1, 1, 512, False), (0, 1, 512, False), (1, 3, 1024, True), (1, 4, 2048, True), (0, 2, 4096, False)} <= seen


@pytest.mark.parametrize("combo", F.ANCHORED, ids=_id)
def test_dense_case_against_the_exact_sum(gpu, capfd, monkeypatch, combo):
    name, eps, sigma = combo
    R.check(np.array(_default(combo, capfd, monkeypatch)[0]), name, eps, sigma, path="fft stage, default")


# ---------------------------------------------------------------------------------------------------------------------
# The differential
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def children(gpu, tmp_path_factory):
    """The other realisations, one child process after another (never two at once, nothing retried), each with its own
    time limit; the first child that does not exit 0 ends the fixture.  label -> (results by combination, passes by
    combination, refused combinations)."""
    from tests.fft_stage_worker import MARK

    res = {}
    tmp = tmp_path_factory.mktemp("fft_stage")
    for label, switch in F.REALISATIONS.items():
        out = tmp / f"{label}.npz"
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(switch, PYTHONPATH=ROOT, FFTVIS_HIP_DEBUG_FFT="1")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fft_stage_worker.py"), str(out)], env=env,
                           capture_output=True, text=True, timeout=420)
        if r.returncode != 0:
            pytest.fail(f"realisation {label} ended with status {r.returncode}; none started after it\n"
                        + r.stdout[-2000:] + r.stderr[-4000:])
        z = np.load(out)
        refused = {F.COMBOS[int(i)]: why for i, why in json.loads(str(z["refused"])).items()}
        passes = {}
        for chunk in r.stderr.split(MARK)[1:]:
            passes[F.COMBOS[int(chunk.split()[0])]] = F.parse_debug(chunk)
        res[label] = ({c: z[f"r{i}"] for i, c in enumerate(F.COMBOS) if c not in refused}, passes, refused)
        _log({"path": "realisation", "label": label, "refused": [list(c) + [w] for c, w in refused.items()]})
    return res


@pytest.mark.parametrize("combo", F.COMBOS, ids=_id)
def test_realisations_differ_by_fft_rounding_only(gpu, capfd, monkeypatch, children, combo):
    """Default against each other realisation that ran the combination, and (to name the odd one out when one fails) the
    others against the old kernel."""
    name, eps, sigma = combo
    runs = {"default": np.array(_default(combo, capfd, monkeypatch)[0])}
    runs.update({label: got[combo] for label, (got, _, refused) in children.items() if combo not in refused})
    assert len(runs) >= 2, (combo, {label: r[2].get(combo) for label, r in children.items()})
    Z, bad, worst = F.z_case(name, eps, sigma), [], {}
    pairs = [("default", lb) for lb in runs if lb != "default"]
    pairs += [(lb, "old_fft") for lb in runs if lb not in ("default", "old_fft") and "old_fft" in runs]
    for a, b in pairs:
        ok, w, K = F.diff_ok(runs[a], runs[b], name, eps, sigma)
        worst[f"{a}|{b}"] = w
        if not ok:
            bad.append((a, b, w))
    _log({"case": name, "eps": eps, "sigma": sigma, "path": "differential", "Z_case": Z, "K": 4.0 * max(Z, 1.0),
          "worst_D_in_fft_terms": worst, "precision": R.case(name)["precision"]})
    assert not bad, (combo, "K", 4.0 * max(Z, 1.0), worst)


def test_old_kernel_refusals_are_the_known_ones(gpu, children):
    """Which combinations a realisation refused (an argument error before any launch) is part of the record: none today."""
    assert {label: sorted(r[2]) for label, r in children.items() if r[2]} == {}


def test_children_ran_the_plans_their_switches_ask_for(gpu, children):
    """FFTVIS_HIP_PAIR=2 pairs the residues of every folded Q = 1024 / 2048 pass of the register-resident kernel (row mode:
    where a workgroup holds two rows); FFTVIS_HIP_PAIR=0 and the natural order launch the default factorisation."""
    npaired = 0
    for combo in F.COMBOS:
        name, eps, sigma = combo
        want = F.plan(name, eps, sigma)
        got = children["pair2"][1][combo]
        pair = tuple(int(g["st"] and g["folded"] and g["P"] >= 2 and g["Q"] in (1024, 2048) and (g["col"] == 1 or p["rpw"] >= 2))
                     for g, p in zip(want, got))
        npaired += sum(pair)
        _same_plan(got, name, eps, sigma, pair)
        _same_plan(children["pair0"][1][combo], name, eps, sigma)
        _same_plan(children["natural_order"][1][combo], name, eps, sigma)
    assert npaired >= 8, npaired
