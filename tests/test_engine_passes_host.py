"""CPU tests of ``GPUSimulationEngine.simulate`` end to end against a recording handle: which pass a call's mode keyword
selects, what the handle is told and in which order, how the time blocks are walked, how the mode keywords exclude each
other, and when the handle is returned or closed.  ``_acquire_handle`` hands out the fake, ``_time_block`` answers 2, and
the buffers are numpy arrays, so no GPU is touched.  (The passes that allocate device tensors -- ``objective_of``,
``gauss_newton_of``, ``forward_to`` -- have their block behaviour pinned on the GPU.)

The plain runs are ``synth.make_config("C1", nsrc=5, nfreq=2, ntimes=3)``: hera7 on its lattice, 21 baselines, 3 time steps
in blocks (0, 2) and (2, 3); the basis runs ``basis_source_refs.basis_source_config`` at the same sizes: 30 baselines,
K = 3, polarized.
"""

import itertools

import numpy as np
import pytest

from fftvis_amd import synth
from fftvis_amd.gpu import gpu_simulate
from fftvis_amd.gpu.gpu_simulate import GPUSimulationEngine
from tests.basis_source_refs import basis_source_config

NSRC, NF, NT = 5, 2, 3
MODES = ("adjoint_of", "tangent_of", "basis_tangent_of", "basis_source_of", "sky_of", "objective_of", "gauss_newton_of",
         "forward_to")
SETUP = ["set_sources", "set_times", "set_freqs", "set_array_type1", "set_beams", "set_chunking", "set_reference_compat",
         "set_beam_pairs"]


def describe(x):
    """An argument as the expected lists write it: scalars as they are, an array as its shape, anything else by type."""
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return tuple(x.shape) if isinstance(x, np.ndarray) else type(x).__name__


class RecordingHandle:
    """What ``simulate`` asks of a ``SimHandle``, in order: (name, described arguments...).  ``fail`` names a method that
    raises."""

    def __init__(self, precision, polarized, fail=None, describe=describe):
        self.rdt, self.cdt = (np.float32, np.complex64) if precision == 1 else (np.float64, np.complex128)
        self.polarized, self.fail, self.describe, self.calls, self.nbls = polarized, fail, describe, [], 0

    def out_shape(self, nt, nf):
        return (nf, nt, 2, 2, self.nbls) if self.polarized else (nf, nt, self.nbls)

    def record(self, name, *args, **kw):
        if name == self.fail:
            raise RuntimeError(f"{name} failed")
        self.calls.append((name,) + tuple(self.describe(a) for a in args) + tuple(
            (k, self.describe(v)) for k, v in kw.items()))

    def set_array(self, R, bls, is_coplanar):
        self.nbls = bls.shape[1]
        self.record("set_array", R, bls, is_coplanar)

    def set_array_type1(self, basis_matrix, bls_int, n_modes):
        self.nbls = bls_int.shape[1]
        self.record("set_array_type1", basis_matrix, bls_int, n_modes)

    def run(self, t0, t1, f0, f1, out=None, shared=False):
        self.record("run", t0, t1, f0, f1)
        if out is None:
            return np.zeros(self.out_shape(t1 - t0, f1 - f0), self.cdt)
        out[...] = 0
        return out

    def close(self):
        self.record("close")

    def __getattr__(self, name):
        if not name.startswith(("set_", "run_")):
            raise AttributeError(name)
        return lambda *args, **kw: self.record(name, *args, **kw)


class Mgr:
    """A matvis-style manager of ``NSRC`` sources whose vectors at time index ti are all ti."""

    def setup(self):
        pass

    def rotate(self, ti):
        self.all_coords_topo = np.full((3, NSRC), float(ti))


class Engine:
    """``simulate`` on the CPU: every handle asked for is a ``RecordingHandle``; ``sized`` collects the channel counts
    ``_time_block`` was asked about, ``returned`` the handles given back."""

    def __init__(self, monkeypatch, fail=None, describe=describe):
        self.handles, self.returned, self.sized = [], [], []

        def acquire(device, precision, eps, upsample_factor, polarized):
            self.handles.append(RecordingHandle(precision, polarized, fail, describe))
            return "key", self.handles[-1]

        def time_block(device, nt, nf, *rest):
            self.sized.append(nf)
            return 2

        monkeypatch.setattr(gpu_simulate, "_acquire_handle", acquire)
        monkeypatch.setattr(gpu_simulate, "_return_handle", lambda key, h: self.returned.append(h))
        monkeypatch.setattr(gpu_simulate, "_time_block", time_block)

    def __call__(self, cfg, **kw):
        cfg = dict(cfg, **kw)
        beam = cfg.pop("beam")
        return GPUSimulationEngine().simulate(beam_list=list(beam) if isinstance(beam, list) else [beam], **cfg)

    @property
    def calls(self):
        (h,) = self.handles
        return h.calls

    def names(self, prefix):
        return [c[0] for c in self.calls if c[0].startswith(prefix)]

    def runs(self):
        return [c for c in self.calls if c[0].startswith("run")]


@pytest.fixture
def engine(monkeypatch):
    return Engine(monkeypatch)


def plain(**kw):
    return dict(synth.make_config("C1", nsrc=NSRC, nfreq=NF, ntimes=NT), **dict({"force_use_type3": False}, **kw))


def basis(**kw):
    return dict(basis_source_config(nsrc=NSRC, nfreq=NF, ntimes=NT), **kw)


NBLS, NBLS_BASIS = 21, 30
G = np.zeros((NF, NT, NBLS), complex)
G_BASIS = np.zeros((NF, NT, 2, 2, NBLS_BASIS), complex)


def test_forward_on_the_lattice_array(engine):
    vis = engine(plain())
    assert vis.shape == (NF, NT, NBLS) and vis.dtype == np.complex128
    assert engine.calls == [
        ("set_sources", (3, NSRC), (NSRC, NF), False), ("set_times", (NT, 3, 3)), ("set_freqs", (NF,)),
        ("set_array_type1", (3, 3), (3, NBLS), 5), ("set_beams", "list", (NF,), 1, "x"), ("set_chunking", 1, 1.0),
        ("set_reference_compat", True), ("set_beam_pairs", "list", "dict", "dict"),
        ("run", 0, 2, 0, NF), ("run", 2, 3, 0, NF)]
    assert engine.returned == engine.handles and engine.sized == [NF]


def test_forward_with_the_type3_transform(engine):
    engine(plain(force_use_type3=True))
    assert engine.names("set_") == SETUP[:3] + ["set_array"] + SETUP[4:]
    assert engine.calls[3] == ("set_array", (3, 3), (3, NBLS), True)
    assert engine.runs() == [("run", 0, 2, 0, NF), ("run", 2, 3, 0, NF)] and len(engine.returned) == 1


def test_forward_with_a_coordinate_manager(engine):
    """No ``set_times``; every block's vectors are streamed before its run, which then counts from 0."""
    engine(plain(coord_mgr=Mgr()))
    assert engine.names("set_")[:7] == [n for n in SETUP if n != "set_times"]
    assert engine.calls[7:] == [("set_topo", (2, 3, NSRC)), ("run", 0, 2, 0, NF), ("set_topo", (1, 3, NSRC)),
                                ("run", 0, 1, 0, NF)]
    assert len(engine.returned) == 1


@pytest.mark.parametrize("kw, path", [
    ({}, "type3"), ({"adjoint_path": "auto"}, "type2"), ({"adjoint_path": "type2"}, "type2"),
    ({"adjoint_path": "auto", "force_use_type3": True}, "type3")])
def test_flux_adjoint_sets_its_path_and_accumulates_after_the_first_block(engine, kw, path):
    gflux = np.ones((NSRC, NF))
    assert engine(plain(**kw), adjoint_of=(G, gflux)) is gflux
    assert engine.names("set_") == SETUP[:3] + ["set_array" if kw.get("force_use_type3") else "set_array_type1"] + SETUP[
        4:] + ["set_adjoint_path"]
    assert engine.calls[8:] == [("set_adjoint_path", path), ("run_adjoint", 0, 2, 0, NF, (NF, 2, NBLS), (NSRC, NF), False),
                                ("run_adjoint", 2, 3, 0, NF, (NF, 1, NBLS), (NSRC, NF), True)]
    assert engine.returned == engine.handles and engine.sized == [NF]


@pytest.mark.parametrize("wrt, who", [("positions", "position"), ("sources", "source")])
def test_position_and_source_adjoints(engine, wrt, who):
    buf = np.ones((NBLS, 3)) if wrt == "positions" else np.ones((NT, NSRC, 3))
    with pytest.raises(ValueError) as e:
        engine(plain(), adjoint_of=(G, buf), adjoint_wrt=wrt)
    assert str(e.value) == f"the {who} adjoint runs the type-3 transform: pass force_use_type3=True on a lattice array"
    assert engine.handles == []
    assert engine(plain(force_use_type3=True), adjoint_of=(G, buf), adjoint_wrt=wrt) is buf
    assert engine.calls[8] == ("set_adjoint_path", "type3")
    if wrt == "positions":
        assert engine.runs() == [("run_position_adjoint", 0, 2, 0, NF, (NF, 2, NBLS), (NBLS, 3), False),
                                 ("run_position_adjoint", 2, 3, 0, NF, (NF, 1, NBLS), (NBLS, 3), True)]
    else:  # every block fills its own rows: nothing accumulates
        assert engine.runs() == [("run_source_adjoint", 0, 2, 0, NF, (NF, 2, NBLS), (2, NSRC, 3), False),
                                 ("run_source_adjoint", 2, 3, 0, NF, (NF, 1, NBLS), (1, NSRC, 3), False)]
    assert len(engine.returned) == 1


def test_tangent(engine):
    dbls, dtopo, dv = np.zeros((NBLS, 3)), np.zeros((NT, NSRC, 3)), np.zeros(G.shape, complex)
    with pytest.raises(ValueError, match="the tangent runs the type-3 transform: pass force_use_type3=True on a lattice"):
        engine(plain(), tangent_of=(dbls, dtopo, dv))
    assert engine.handles == []
    assert engine(plain(force_use_type3=True), tangent_of=(dbls, dtopo, dv)) is dv
    assert engine.names("set_") == SETUP[:3] + ["set_array"] + SETUP[4:]  # (no adjoint path)
    assert engine.runs() == [("run_tangent", 0, 2, 0, NF, (NBLS, 3), (2, NSRC, 3), (NF, 2, NBLS)),
                             ("run_tangent", 2, 3, 0, NF, (NBLS, 3), (1, NSRC, 3), (NF, 1, NBLS))]


BASIS_SETUP = ["set_sources", "set_times", "set_freqs", "set_array", "set_beams", "set_chunking", "set_reference_compat",
               "set_basis"]


def test_position_tangent_through_basis_beams(engine):
    dbls, dv = np.zeros((NBLS_BASIS, 3)), np.zeros(G_BASIS.shape, complex)
    assert engine(basis(), tangent_of=(dbls, None, dv)) is dv
    assert engine.names("set_") == BASIS_SETUP
    assert engine.calls[7] == ("set_basis", (7, 3, NF), (NBLS_BASIS,), (NBLS_BASIS,))
    assert engine.runs() == [("run_basis_position_tangent", 0, 2, 0, NF, (NBLS_BASIS, 3), (NF, 2, 2, 2, NBLS_BASIS)),
                             ("run_basis_position_tangent", 2, 3, 0, NF, (NBLS_BASIS, 3), (NF, 1, 2, 2, NBLS_BASIS))]


def test_basis_tangent_sizes_its_blocks_for_every_direction(engine):
    dcoefs, dv = np.zeros((3, 7, 3, NF), complex), np.zeros((3,) + G_BASIS.shape, complex)
    assert engine(basis(), basis_tangent_of=(dcoefs, dv)) is dv
    assert engine.sized == [NF * 3] and engine.names("set_") == BASIS_SETUP
    assert engine.runs() == [("run_basis_tangent", 0, 2, 0, NF, (3, 7, 3, NF), (3, NF, 2, 2, 2, NBLS_BASIS)),
                             ("run_basis_tangent", 2, 3, 0, NF, (3, 7, 3, NF), (3, NF, 1, 2, 2, NBLS_BASIS))]


def test_basis_source_passes(engine, monkeypatch):
    gtopo = np.ones((NT, NSRC, 3))
    assert engine(basis(), basis_source_of=("adjoint", G_BASIS, gtopo)) is gtopo
    assert engine.names("set_") == BASIS_SETUP
    assert engine.runs() == [("run_basis_source_adjoint", 0, 2, 0, NF, (NF, 2, 2, 2, NBLS_BASIS), (2, NSRC, 3), False),
                             ("run_basis_source_adjoint", 2, 3, 0, NF, (NF, 1, 2, 2, NBLS_BASIS), (1, NSRC, 3), False)]
    engine = Engine(monkeypatch)
    dv = np.zeros(G_BASIS.shape, complex)
    assert engine(basis(), basis_source_of=("tangent", gtopo, dv)) is dv
    assert engine.runs() == [("run_basis_source_tangent", 0, 2, 0, NF, (2, NSRC, 3), (NF, 2, 2, 2, NBLS_BASIS)),
                             ("run_basis_source_tangent", 2, 3, 0, NF, (1, NSRC, 3), (NF, 1, 2, 2, NBLS_BASIS))]
    assert len(engine.returned) == 1


@pytest.mark.parametrize("with_basis", [False, True])
def test_sky_adjoint(engine, with_basis):
    cfg, g = (basis(), G_BASIS) if with_basis else (plain(force_use_type3=True), G)
    gflux, gtopo = np.ones((NSRC, NF)), np.ones((NT, NSRC, 3))
    out = engine(cfg, sky_of=(g, gflux, gtopo))
    assert out[0] is gflux and out[1] is gtopo
    assert engine.names("set_") == (BASIS_SETUP if with_basis else SETUP[:3] + ["set_array"] + SETUP[4:])
    blk = (lambda n: (NF, n, 2, 2, NBLS_BASIS)) if with_basis else (lambda n: (NF, n, NBLS))
    assert engine.runs() == [
        ("run_sky_adjoint", 0, 2, 0, NF, blk(2), (NSRC, NF), (2, NSRC, 3), False, ("basis", with_basis)),
        ("run_sky_adjoint", 2, 3, 0, NF, blk(1), (NSRC, NF), (1, NSRC, 3), True, ("basis", with_basis))]
    if not with_basis:
        with pytest.raises(ValueError, match="the sky adjoint runs the type-3 transform: pass force_use_type3=True on a "):
            engine(plain(), sky_of=(g, gflux, gtopo))
        assert len(engine.handles) == 1


@pytest.mark.parametrize("with_gbls", [False, True])
def test_adjoint_through_basis_beams(engine, with_gbls):
    """No adjoint path is set; with ``gbls`` the position pass follows the other two in every block."""
    gflux, gcoefs, gbls = np.ones((NSRC, NF)), np.ones((7, 3, NF), complex), np.ones((NBLS_BASIS, 3))
    out = engine(basis(), adjoint_of=(G_BASIS, gflux, gcoefs) + ((gbls,) if with_gbls else ()))
    assert out[0] is gflux and out[1] is gcoefs and len(out) == (3 if with_gbls else 2)
    assert engine.names("set_") == BASIS_SETUP
    expected = []
    for (ta, te), acc in (((0, 2), False), ((2, 3), True)):
        blk = (NF, te - ta, 2, 2, NBLS_BASIS)
        expected.append(("run_basis_adjoint", ta, te, 0, NF, blk, (NSRC, NF), (7, 3, NF), acc))
        if with_gbls:
            expected.append(("run_basis_position_adjoint", ta, te, 0, NF, blk, (NBLS_BASIS, 3), acc))
    assert engine.runs() == expected and len(engine.returned) == 1


PAYLOADS = dict(
    adjoint_of=(G, np.zeros((NSRC, NF))), tangent_of=(np.zeros((NBLS, 3)), None, np.zeros(G.shape, complex)),
    basis_tangent_of=(np.zeros((1, 7, 3, NF), complex), np.zeros((1,) + G.shape, complex)),
    basis_source_of=("adjoint", G, np.zeros((NT, NSRC, 3))), sky_of=(G, np.zeros((NSRC, NF)), np.zeros((NT, NSRC, 3))),
    objective_of=(G, None, {}), gauss_newton_of=({"d_fluxes": np.zeros((NSRC, NF))}, None, {}), forward_to=True)
PINNED = {
    ("adjoint_of", "tangent_of"): "pass either adjoint_of or tangent_of, not both",
    ("adjoint_of", "basis_tangent_of"): "pass one of adjoint_of, tangent_of and basis_tangent_of",
    ("tangent_of", "basis_source_of"): "pass one of adjoint_of, tangent_of, basis_tangent_of and basis_source_of",
    ("adjoint_of", "sky_of"): "pass one of adjoint_of, tangent_of, basis_tangent_of, basis_source_of and sky_of",
    ("sky_of", "objective_of"): "pass one of adjoint_of, tangent_of, basis_tangent_of, basis_source_of, sky_of and "
                                "objective_of",
    ("objective_of", "gauss_newton_of"): "pass one of adjoint_of, tangent_of, basis_tangent_of, basis_source_of, sky_of, "
                                         "objective_of and gauss_newton_of",
    ("adjoint_of", "forward_to"): "forward_to is the plain forward run: no other pass and no out= with it",
    ("gauss_newton_of", "forward_to"): "forward_to is the plain forward run: no other pass and no out= with it",
}


@pytest.mark.parametrize("first, second", list(itertools.combinations(MODES, 2)))
def test_two_mode_keywords_are_refused_before_a_handle_is_acquired(engine, first, second):
    """The message is the later keyword's: it lists the keywords that came before it."""
    with pytest.raises(ValueError) as e:
        engine(plain(), **{first: PAYLOADS[first], second: PAYLOADS[second]})
    assert engine.handles == []
    earlier = MODES[:MODES.index(second)]
    assert all(m in str(e.value) for m in earlier + (second,)) or second == "forward_to"
    if (first, second) in PINNED:
        assert str(e.value) == PINNED[(first, second)]


def test_forward_to_takes_no_out(engine):
    with pytest.raises(ValueError, match="forward_to is the plain forward run: no other pass and no out= with it"):
        engine(plain(), forward_to=True, out=np.zeros(G.shape, complex))
    assert engine.handles == []


def test_a_failing_run_closes_the_handle_and_does_not_return_it(monkeypatch):
    engine = Engine(monkeypatch, fail="run_adjoint")
    with pytest.raises(RuntimeError, match="run_adjoint failed"):
        engine(plain(), adjoint_of=(G, np.zeros((NSRC, NF))))
    assert engine.calls[-1] == ("close",) and engine.returned == []
    engine = Engine(monkeypatch)  # a successful run: returned once, never closed
    engine(plain(), adjoint_of=(G, np.zeros((NSRC, NF))))
    assert engine.returned == engine.handles and "close" not in engine.names("")
