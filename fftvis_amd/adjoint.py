"""Adjoint of ``simulate_vis`` with respect to ``fluxes``, and a torch autograd entry point.

``simulate_vis`` is linear in ``fluxes``: V = A F.  The adjoint is taken for the REAL inner products

    Re <A F, G> = <F, A^T G>      for every real F and complex G,

because the map is real-linear, not complex-linear (flipped two-beam baselines are conjugated, fluxes are real Stokes
parameters).  ``A^T G`` has the shape of ``fluxes``.  The device computes it per (time, frequency group, beam pair)
with the roles of the forward's type-3 transform swapped (``fv_sim_run_adjoint``, DESIGN.md "Adjoint"); on lattice arrays
``adjoint_path="type2"`` takes the transpose of the type-1 slice instead, a type-2 transform.

Basis beams (``beam_coefs``) have entry points of their own, ``simulate_vis_basis_adjoint`` and ``torch_simulate_vis_basis``:
the same adjoint with respect to the fluxes, and the gradient with respect to the coefficients, in which the map is
sesquilinear (``fv_sim_run_basis_adjoint``).

The antenna positions have theirs as well, ``simulate_vis_position_adjoint`` and ``torch_simulate_vis_array``: the
gradient of the exact sum every forward path approximates, from forward transforms of the strengths times the sources'
coordinates (``fv_sim_run_position_adjoint``).

The other product, J v, is ``simulate_vis_jvp``: the forward-mode tangent of the visibilities along a change of the
antenna positions, the source positions and the fluxes (``fv_sim_run_tangent``), which the three torch operations
also offer to ``torch.autograd.forward_ad`` through their ``jvp``.  Basis beams have their own,
``simulate_vis_basis_jvp``: the tangent along directions of the coefficients and of the fluxes
(``fv_sim_run_basis_tangent``), several directions per call, and the ``jvp`` of ``torch_simulate_vis_basis``.

A fit's G is 2 w (V - d).  ``simulate_vis_chi2`` and ``torch_simulate_vis_chi2`` form it on the device, behind the forward
run of the same handle (``fv_sim_run_residual``), and run the passes above on it where it lies: chi2 and its gradients
from one call, one set-up, with the visibilities never copied to the host.  ``simulate_vis_gain_chi2`` is that
call with ``gains=``: the data model is conj(g[a1]) g[a2] V, one complex gain per antenna, feed, channel and optionally time, applied on the device in the same
block (``fv_sim_run_residual_gains``), and ``wrt="gains"`` gives the gradient with respect to them.
``simulate_vis_jones_chi2`` takes a full 2 x 2 matrix per antenna instead -- the two gains and the leakage between the
feeds -- with ``wrt="jones"`` (``fv_sim_run_residual_jones``).
``simulate_vis_gauss_newton`` is the Gauss-Newton product 2 J^T W J p of that chi2 from one call that keeps the tangent on
the device (``fv_sim_weight_block``), and ``simulate_vis_gain_gauss_newton`` that product with the gains in the data model,
a gain direction and the gain block of the product (``fv_sim_gain_weight_block``); ``simulate_vis_jones_gauss_newton`` is
the same with 2 x 2 matrices and a direction of such matrices (``fv_sim_jones_weight_block``).  ``simulate_vis_gain_solve`` solves
the gains themselves against a fixed model: one forward into a device tensor, or a resident ``model=``, and the alternating
per-antenna solve on the device (``fv_gain_solve``).  ``simulate_vis_jones_solve`` is that solve for the full 2 x 2 matrices
(``fv_jones_solve``).
"""

from __future__ import annotations

import dataclasses

import numpy as np

from .core.beams import feed_index
from .core.coords import julian_dates
from .core.simulate import default_accuracy_dict
from .core.utils import get_pos_reds, validate_beam_idx


def _is_tensor(x) -> bool:
    import sys

    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


# ---- the host layer every pass below shares ("Host layer of the derivative passes") ----

# keywords a pass hands to ``engine.simulate`` and to ``simulate_vis`` as its caller gave them
_PASS_THROUGH = ("ra", "dec", "freqs", "times", "telescope_loc", "precision", "polarized", "upsample_factor",
                 "beam_spline_opts", "use_feed", "flat_array_tol", "interpolation_function", "nprocesses", "nthreads",
                 "coord_method", "coord_method_params", "force_use_ray", "trace_mem", "source_buffer", "coord_mgr",
                 "reference_compat", "device_astrometry")


@dataclasses.dataclass(frozen=True)
class _Run:
    """One call of a pass: the arguments as given (``args``: the public function's ``locals()``), and what every pass
    derives from them before any device work."""

    args: dict
    ants: dict
    beam_list: list
    beam_idx: np.ndarray
    beam_coefs: np.ndarray  # on the host; None without basis beams
    baselines: list
    eps: float
    astrom: np.ndarray
    nsrc: int
    nfreqs: int
    ntimes: int
    nbls: int
    rdt: type
    cdt: type
    vis_shape: tuple

    def dtype(self, kind):
        """numpy dtype of a buffer: "real" and "complex" of the run's precision, or "float64"."""
        return {"real": self.rdt, "complex": self.cdt, "float64": np.float64}[kind]


def _describe_run(args) -> _Run:
    """The run a pass's arguments describe, normalised as ``simulate_vis`` normalises them; ValueError for what no run
    takes.  A pass that refuses ``beam_coefs`` does so before: here they mean basis beams."""
    if args["backend"] != "gpu":
        raise ValueError(f"Unsupported backend: {args['backend']}")
    precision, polarized = args["precision"], args["polarized"]
    ants = {k: np.array(v) for k, v in args["ants"].items()}
    beam = args["beam"]
    beam_list = list(beam) if isinstance(beam, (list, tuple)) else [beam]
    beam_coefs = None if args["beam_coefs"] is None else _host(args["beam_coefs"])
    beam_idx = validate_beam_idx(args["beam_idx"], beam_coefs, len(beam_list), len(ants))
    feed_index(args["use_feed"])
    baselines = args["baselines"]
    if baselines is None:
        baselines = [red[0] for red in get_pos_reds(ants, include_autos=True)]
    nfreqs, ntimes, nbls = int(np.size(args["freqs"])), len(julian_dates(args["times"])), len(baselines)
    if beam_coefs is not None and beam_coefs.shape != (len(ants), len(beam_list), nfreqs):
        raise ValueError("beam_coefs must have shape (nant, nbasis, nfreqs)")
    return _Run(
        args=args, ants=ants, beam_list=beam_list, beam_idx=beam_idx, beam_coefs=beam_coefs, baselines=baselines,
        eps=default_accuracy_dict[precision] if args["eps"] is None else args["eps"], astrom=args["astrom"],
        nsrc=int(np.size(args["ra"])), nfreqs=nfreqs, ntimes=ntimes, nbls=nbls,
        rdt=np.float32 if precision == 1 else np.float64, cdt=np.complex64 if precision == 1 else np.complex128,
        vis_shape=(nfreqs, ntimes, 2, 2, nbls) if polarized else (nfreqs, ntimes, nbls),
    )


def _shared_keywords(run: _Run) -> dict:
    """What ``engine.simulate`` and ``simulate_vis`` take alike."""
    return dict({k: run.args[k] for k in _PASS_THROUGH}, ants=run.ants, beam_idx=run.beam_idx, baselines=run.baselines,
                eps=run.eps, astrom=run.astrom)


def _engine_simulate(run: _Run, fluxes, *, force_use_type3=None, **mode):
    """One ``engine.simulate`` call of the run on the host array ``fluxes``; ``mode`` is the pass's own keyword
    (``adjoint_of=``, ``tangent_of=``, ...).  ``force_use_type3`` defaults to the caller's."""
    from .wrapper import create_simulation_engine, device_chunks

    a = run.args
    nfeed = 2 if a["polarized"] else 1
    engine = create_simulation_engine(backend=a["backend"], device=a["device"])
    nchunks = device_chunks(a["device"], a["max_memory"], a["min_chunks"], run.beam_list, nfeed, nfeed, len(run.ants),
                            run.nsrc, a["precision"], a["source_buffer"], run.nfreqs)
    return engine.simulate(
        fluxes=fluxes.astype(run.rdt, copy=False), beam_list=run.beam_list, nchunks=nchunks,
        beam_coefs=None if run.beam_coefs is None else run.beam_coefs.astype(run.cdt, copy=False),
        force_use_type3=a["force_use_type3"] if force_use_type3 is None else force_use_type3,
        **_shared_keywords(run), **mode)


def _forward_simulate(run: _Run, fluxes, out):
    """Add ``simulate_vis`` of the run on the fluxes' tangent to ``out``: the map is linear in the fluxes."""
    from .wrapper import simulate_vis

    a = run.args
    vf = simulate_vis(fluxes=_host(fluxes).astype(run.rdt, copy=False), beam=run.beam_list, beam_coefs=run.beam_coefs,
                      force_use_type3=a["force_use_type3"], backend=a["backend"], max_memory=a["max_memory"],
                      min_chunks=a["min_chunks"], device=a["device"], **_shared_keywords(run))
    if _is_tensor(out):
        import torch

        vf = torch.from_numpy(np.ascontiguousarray(vf)).to(out.device)
    out += vf


def _host(x) -> np.ndarray:
    """An array or a tensor as a host array (a lazily conjugated or negated view's memory is not its value)."""
    return x.detach().resolve_conj().resolve_neg().cpu().numpy() if _is_tensor(x) else np.asarray(x)


def _on(device, x, dtype):
    """``x`` as a contiguous tensor of the numpy ``dtype`` on the torch ``device``, for the library to read by pointer."""
    import torch

    x = x.detach() if _is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=getattr(torch, np.dtype(dtype).name)).resolve_conj().resolve_neg().contiguous()


def _zeros(device, shape, dtype):
    """A zeroed buffer: a tensor on the torch ``device``, a numpy array when that is None."""
    if device is None:
        return np.zeros(shape, dtype=dtype)
    import torch

    return torch.zeros(shape, dtype=getattr(torch, np.dtype(dtype).name), device=device)


def _synchronize(device):
    """The library's streams do not follow torch's: what torch queued on ``device`` (inputs, zeroed outputs) is complete
    before the library touches it."""
    if device is not None:
        import torch

        torch.cuda.synchronize(device)


def _run_device(run: _Run, tensors, what):
    """The torch device the run's buffers live on: that of the first device tensor among ``tensors``, None when there is
    none (host buffers).  ``what`` names it in the error when it is not the run's device."""
    t = next((x for x in tensors if _is_tensor(x) and x.device.type == "cuda"), None)
    if t is None:
        return None
    if (t.device.index or 0) != int(run.args["device"]):
        raise ValueError(f"{what} lives on {t.device}, the run is on cuda:{int(run.args['device'])}")
    return t.device


def _gradient_buffers(run: _Run, vis, wanted):
    """``vis`` as the library reads it and one zeroed output per entry of ``wanted`` -- (shape, "real" | "complex" |
    "float64"), or None for an output not asked for: tensors on ``vis``' device for a device tensor (complete before the
    call returns), numpy arrays otherwise.  Returns (g, outputs, on_device)."""
    if tuple(vis.shape) != run.vis_shape:
        raise ValueError(f"vis must have simulate_vis's output shape {run.vis_shape}, got {tuple(vis.shape)}")
    device = _run_device(run, (vis,), "vis")
    g = _host(vis).astype(run.cdt, copy=False) if device is None else _on(device, vis, run.cdt)
    outs = [None if w is None else _zeros(device, w[0], run.dtype(w[1])) for w in wanted]
    _synchronize(device)
    return g, outs, device is not None


def _buffer(run: _Run, device, x, kind):
    """A tangent as the library reads it: None stays None."""
    if x is None:
        return None
    return np.ascontiguousarray(_host(x), dtype=run.dtype(kind)) if device is None else _on(device, x, run.dtype(kind))


def _host_fluxes(run: _Run, fluxes, d_fluxes=None) -> np.ndarray:
    """The forward's fluxes as a host array, checked against the catalog (and their tangent's shape against theirs)."""
    fluxes = _host(fluxes)
    if fluxes.shape not in ((run.nsrc, run.nfreqs), (run.nsrc, run.nfreqs, 4)):
        raise ValueError("fluxes must have shape (nsources, nfreqs[, 4])")
    if fluxes.ndim == 3 and not run.args["polarized"]:
        raise ValueError("a full-Stokes sky needs polarized=True")
    if d_fluxes is not None and tuple(d_fluxes.shape) != fluxes.shape:
        raise ValueError(f"d_fluxes must have fluxes' shape {fluxes.shape}, got {tuple(d_fluxes.shape)}")
    return fluxes


def _baseline_tangent(run: _Run, d_ants, d_baselines):
    """The baselines' tangent from ``d_ants`` or ``d_baselines`` (not both), (nbls, 3) or None."""
    if d_ants is not None and d_baselines is not None:
        raise ValueError("give the antenna tangent as d_ants or as d_baselines, not both")
    if d_ants is not None:
        d_baselines = antenna_to_baseline_tangent(d_ants, run.ants, run.baselines)
    if d_baselines is not None and tuple(d_baselines.shape) != (run.nbls, 3):
        raise ValueError(f"d_baselines must have shape ({run.nbls}, 3), got {tuple(d_baselines.shape)}")
    return d_baselines


def _parse_wrt(wrt, allowed, describe):
    """``wrt`` -- a name or a tuple of distinct names out of ``allowed`` -- as (single, names)."""
    single = isinstance(wrt, str)
    names = (wrt,) if single else tuple(wrt)
    if not names or any(n not in allowed for n in names) or len(set(names)) != len(names):
        raise ValueError(f"wrt must name {describe}, got {wrt!r}")
    return single, names


def _select(res: dict, single, names, like, on_device):
    """The gradients asked for out of ``res``, in ``wrt``'s order; a host tensor (``like``) in, host tensors out."""
    if _is_tensor(like) and not on_device:
        import torch

        res = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in res.items()}
    return res[names[0]] if single else tuple(res[n] for n in names)


def _own_radec_chain(run: _Run, asked, needed, with_mgr, with_matvis) -> _Run:
    """For a pass that chains (ra, dec) to the topocentric vectors itself (``needed``; ``asked`` names the argument that
    asks for it): ValueError where the chain is a coordinate manager's, with the pass's advice.  Under device astrometry
    the run gets its contexts here, so that the engine and ``radec_jacobian`` see the same."""
    a = run.args
    own_rotation = a["coord_method"] == "SiderealRotation"
    if needed:
        if a["coord_mgr"] is not None:
            raise ValueError(f"{asked} needs this package's own chain from (ra, dec) to the topocentric vectors; with "
                             f"coord_mgr= the chain is the manager's: {with_mgr}")
        if run.astrom is None and not a["device_astrometry"] and not own_rotation:
            raise ValueError(f"{asked} needs coord_method='SiderealRotation' or device astrometry (astrom= / "
                             f"device_astrometry=True); coord_method={a['coord_method']!r} builds a matvis manager whose "
                             f"chain is its own: {with_matvis}")
    if run.astrom is None and a["device_astrometry"] and a["coord_mgr"] is None and not own_rotation:
        from .core.coords import erfa_astrom_context

        return dataclasses.replace(run, astrom=erfa_astrom_context(a["times"], a["telescope_loc"]))
    return run


def _radec_jacobian_of(run: _Run):
    """``radec_jacobian`` where the run is: the engine rounds ra / dec to the run's precision first."""
    a = run.args
    return radec_jacobian(np.asarray(a["ra"]).astype(run.rdt), np.asarray(a["dec"]).astype(run.rdt), a["times"],
                          a["telescope_loc"], astrom=run.astrom, device=a["device"])


def simulate_vis_adjoint(
    vis,
    ants: dict,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    full_stokes: bool = False,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    beam_coefs: np.ndarray = None,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
    adjoint_path: str = "type3",
):
    """``A^T vis``: the transpose of ``simulate_vis``'s map from ``fluxes`` to visibilities, for the same arguments.

    ``vis`` has ``simulate_vis``'s output shape -- (nfreqs, ntimes, nbls), polarized (nfreqs, ntimes, 2, 2, nbls) -- as a
    numpy array or as a torch tensor on the run's device (handed to the library by pointer, no host copy).  The result
    F satisfies Re <simulate_vis(fluxes), vis> = <fluxes, F> for every real ``fluxes`` and has their shape: (nsrc, nfreqs)
    for Stokes I, (nsrc, nfreqs, 4) with ``full_stokes=True`` (polarized runs only); real, of the run's precision,
    numpy for numpy input and a tensor on ``vis``' device for a tensor.  Every other keyword means what it means for
    ``simulate_vis``, ``reference_compat`` included.  ``adjoint_path`` chooses the transform on lattice arrays, where
    ``simulate_vis`` takes the type-1 transform: ``"type3"`` (default) the type-3 transform with the roles swapped, as on
    every other array; ``"type2"`` the transpose of the type-1 slice itself, a type-2 transform (ValueError when the same
    arguments would not take the lattice path -- not griddable, not flat, ``force_use_type3=True`` -- never a silent
    fall-back); ``"auto"`` type 2 exactly where the forward takes type 1 and type 3 elsewhere.  All compute the same map
    to ``eps``.  Sources below the horizon at every time get exactly 0.  Not covered: ``beam_coefs``
    (NotImplementedError), a sharded multi-GPU adjoint.
    """
    args = locals()
    if adjoint_path not in ("type3", "type2", "auto"):
        raise ValueError(f"adjoint_path must be 'type3', 'type2' or 'auto', got {adjoint_path!r}")
    if beam_coefs is not None:
        raise NotImplementedError("simulate_vis_adjoint does not support basis beams (beam_coefs)")
    if full_stokes and not polarized:
        raise ValueError("full_stokes=True needs polarized=True (a full-Stokes sky needs a polarized simulation)")
    run = _describe_run(args)
    f_shape = (run.nsrc, run.nfreqs)
    g, (gflux,), on_device = _gradient_buffers(
        run, vis, [(f_shape + (2, 2), "complex") if full_stokes else (f_shape, "real")])
    # the catalog's shape is all the engine needs of the fluxes
    fluxes = np.zeros(f_shape + (4,) if full_stokes else f_shape, dtype=run.rdt)
    gc = _engine_simulate(run, fluxes, adjoint_of=(g, gflux), adjoint_path=adjoint_path)
    return _select({"fluxes": stokes_adjoint(gc, full_stokes)}, True, ("fluxes",), vis, on_device)


def stokes_adjoint(gc, full_stokes: bool):
    """Transpose of ``core.utils.prepare_source_catalog`` (Stokes -> coherency, times 0.5): from the gradient with
    respect to the coherency (Re <A C, G> = Re sum conj(gc) C) to the gradient with respect to the Stokes fluxes.
    Stokes I: C = I / 2.  Full Stokes: C = [[I + Q, U + iV], [U - iV, I - Q]] / 2."""
    if not full_stokes:
        return 0.5 * gc
    g00, g01, g10, g11 = gc[..., 0, 0], gc[..., 0, 1], gc[..., 1, 0], gc[..., 1, 1]
    parts = [0.5 * (g00 + g11).real, 0.5 * (g00 - g11).real, 0.5 * (g01 + g10).real, 0.5 * (g01.imag - g10.imag)]
    if _is_tensor(gc):
        import torch

        return torch.stack(parts, dim=-1)
    return np.stack(parts, axis=-1)


_FUNCTIONS = {}


def _function(factory):
    """The ``torch.autograd.Function`` class ``factory`` builds, built on first use: torch is imported only then."""
    if factory not in _FUNCTIONS:
        _FUNCTIONS[factory] = factory()
    return _FUNCTIONS[factory]


def _forward_tensor(kwargs, *, fluxes, **tensors):
    """``simulate_vis(**kwargs)`` on host copies of the operation's tensors, as a tensor on the fluxes' device."""
    import torch

    from .wrapper import simulate_vis

    vis = simulate_vis(fluxes=_host(fluxes), **{k: _host(v) for k, v in tensors.items()}, **kwargs)
    return torch.from_numpy(np.ascontiguousarray(vis)).to(fluxes.device)


def _as_grad(x, device, dtype):
    """A pass's gradient as the tensor autograd expects for an input of that device and dtype; None stays None."""
    import torch

    if x is None:
        return None
    return (x if _is_tensor(x) else torch.from_numpy(x)).to(device=device, dtype=dtype)


def _detached(**tangents):
    """The tangents autograd hands to a ``jvp``, detached; a missing one (None) stays None and skips its part."""
    return {k: None if v is None else v.detach() for k, v in tangents.items()}


def _ants_of(antnums, antpos) -> dict:
    return dict(zip(antnums, antpos.detach().cpu().numpy().astype(np.float64)))


def _checked_antnums(name, antpos, antnums, kwargs) -> tuple:
    """The keys of the rows of the tensor ``antpos`` for the torch operation ``name``, which takes no ``ants=``."""
    if "ants" in kwargs:
        raise TypeError(f"{name} takes the antenna positions as the tensor antpos (and antnums), not ants=")
    if antpos.ndim != 2 or antpos.shape[1] != 3 or antpos.is_complex():
        raise ValueError(f"antpos must be a real (nant, 3) tensor, got {tuple(antpos.shape)} {antpos.dtype}")
    antnums = list(range(antpos.shape[0])) if antnums is None else list(antnums)
    if len(antnums) != antpos.shape[0] or len(set(antnums)) != len(antnums):
        raise ValueError("antnums must give one distinct key per row of antpos")
    return tuple(antnums)


def _autograd_function():
    import torch

    class _SimulateVis(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, kwargs):
            ctx.kwargs = kwargs
            ctx.full_stokes = fluxes.ndim == 3
            ctx.flux_dtype = fluxes.dtype
            # adjoint_path belongs to the backward pass alone
            return _forward_tensor({k: v for k, v in kwargs.items() if k != "adjoint_path"}, fluxes=fluxes)

        @staticmethod
        def backward(ctx, grad_output):
            if not ctx.needs_input_grad[0]:
                return None, None
            g = simulate_vis_adjoint(grad_output, full_stokes=ctx.full_stokes, **ctx.kwargs)
            return _as_grad(g, grad_output.device, ctx.flux_dtype), None

        @staticmethod
        def jvp(ctx, d_fluxes, _):
            # the map is linear in the fluxes: the tangent is the simulation of d_fluxes
            if d_fluxes is None:
                return None
            return _forward_tensor({k: v for k, v in ctx.kwargs.items() if k != "adjoint_path"}, fluxes=d_fluxes)

    return _SimulateVis


def torch_simulate_vis(fluxes, **kwargs):
    """``simulate_vis`` as a differentiable torch operation of ``fluxes`` (a real tensor, (nsrc, nfreqs) or
    (nsrc, nfreqs, 4)); every other argument is a keyword of ``simulate_vis`` (``ants``, ``ra``, ``dec``, ``freqs``,
    ``times``, ``beam``, ``telescope_loc``, ...).  Returns the visibilities as a complex tensor on ``fluxes``' device.
    The backward pass is ``simulate_vis_adjoint`` of the incoming gradient: under torch's convention for a real input
    and a complex output the gradient is Re(A^H g), the adjoint defined there.  ``adjoint_path`` ("type3" | "type2" |
    "auto", see ``simulate_vis_adjoint``) goes to the backward pass only; ``simulate_vis`` never sees it.  Forward mode
    (``torch.autograd.forward_ad``): the map is linear, so the tangent is the simulation of the fluxes' tangent."""
    if kwargs.get("beam_coefs") is not None:
        raise NotImplementedError("torch_simulate_vis does not support basis beams (beam_coefs)")
    if kwargs.get("adjoint_path", "type3") not in ("type3", "type2", "auto"):
        raise ValueError(f"adjoint_path must be 'type3', 'type2' or 'auto', got {kwargs['adjoint_path']!r}")
    return _function(_autograd_function).apply(fluxes, kwargs)


def simulate_vis_basis_adjoint(
    vis,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    beam_coefs,
    telescope_loc,
    *,
    wrt=("fluxes", "beam_coefs"),
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = True,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Gradients of the basis-beam simulation ``simulate_vis(..., beam=<K basis beams>, beam_coefs=C)`` with respect to
    ``fluxes``, to ``beam_coefs`` and to the antenna positions, for a visibility-shaped ``vis`` (G = dL/dV,
    dL = Re sum conj(G) dV).

    * ``"fluxes"``: ``A^T vis`` as ``simulate_vis_adjoint`` defines it, A the map from the fluxes to the visibilities for
      the given coefficients: Re <simulate_vis(F), vis> = <F, result> for every real F; shape and dtype of the fluxes
      ((nsrc, nfreqs), or (nsrc, nfreqs, 4) for a full-Stokes sky).
    * ``"beam_coefs"``: the complex ``gcoefs`` (nant, nbasis, nfreqs) with Re <dV[C; D], vis> = Re <D, gcoefs> for every
      complex direction D, dV[C; D] the derivative of the visibilities along D (they are sesquilinear in C): what torch
      returns for a complex leaf.  It needs ``fluxes``, the forward's input.
    * ``"baselines"``: (nbls, 3) float64, ENU per metre, every listed baseline an independent vector, with the meaning of
      ``simulate_vis_position_adjoint``: every basis visibility M_kl is a sum over sources of strengths that do not depend
      on the positions, so ``gbls[k, d] = -sum_{f,t,r} (2 pi nu_f / c) Im(conj(G) D_d)`` with D_d the basis simulation of
      the fluxes times topo_d (``fv_sim_run_basis_position_adjoint``: about three forward runs whatever the number of
      antennas).  On a coplanar array the up component is still returned.
    * ``"ants"``: (nant, 3) float64, rows in ``ants``' iteration order: ``baseline_to_antenna_gradient`` of the baseline
      result.

    The source positions have a pass of their own, ``simulate_vis_basis_source_adjoint``.  Not covered: a lattice form,
    multi-GPU.

    ``wrt`` names the gradients wanted -- a name, or a tuple of names; the result is that gradient, or a tuple in
    ``wrt``'s order.  Only the passes asked for run; a gradient computed alone equals the one from a joint call bit for
    bit.  ``full_stokes`` defaults to what ``fluxes``' shape says.  ``vis`` is a numpy array or a torch tensor on the run's
    device (handed over by pointer; the results are then tensors on that device); every other argument means what it
    means for ``simulate_vis``, ``reference_compat`` included.  ``polarized`` must be True and ``beam_idx`` None, as for
    the forward."""
    args = locals()
    single, names = _parse_wrt(wrt, ("fluxes", "beam_coefs", "ants", "baselines"),
                               "some of 'fluxes', 'beam_coefs', 'ants' and 'baselines'")
    if beam_coefs is None:
        raise ValueError("simulate_vis_basis_adjoint needs beam_coefs (simulate_vis_adjoint covers per-antenna beam_idx)")
    if not polarized:  # the forward's message
        raise ValueError(
            "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
        )
    run = _describe_run(args)
    fluxes = _host_fluxes(run, fluxes)
    if full_stokes is None:
        full_stokes = fluxes.ndim == 3
    if bool(full_stokes) != (fluxes.ndim == 3):
        raise ValueError(f"full_stokes={full_stokes} does not match fluxes of shape {fluxes.shape}")
    f_shape = (run.nsrc, run.nfreqs)
    g, (gflux, gcoefs, gbls), on_device = _gradient_buffers(run, vis, [
        None if "fluxes" not in names else (f_shape + (2, 2), "complex") if full_stokes else (f_shape, "real"),
        None if "beam_coefs" not in names else (run.beam_coefs.shape, "complex"),
        None if "ants" not in names and "baselines" not in names else ((run.nbls, 3), "float64")])
    # (gflux, gcoefs[, gbls]): the buffers above, filled in place
    gc, gk = _engine_simulate(run, fluxes, adjoint_of=(g, gflux, gcoefs, gbls))[:2]
    res = {"beam_coefs": gk, "baselines": gbls}
    if "fluxes" in names:
        res["fluxes"] = stokes_adjoint(gc, full_stokes)
    if "ants" in names:
        res["ants"] = baseline_to_antenna_gradient(gbls, run.ants, run.baselines)
    return _select({k: v for k, v in res.items() if k in names}, single, names, vis, on_device)


def _basis_autograd_function():
    import torch

    class _SimulateVisBasis(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, beam_coefs, kwargs):
            ctx.kwargs = kwargs
            ctx.flux_dtype, ctx.coef_dtype = fluxes.dtype, beam_coefs.dtype
            ctx.coef_device = beam_coefs.device
            ctx.save_for_backward(fluxes, beam_coefs)
            ctx.save_for_forward(fluxes, beam_coefs)
            return _forward_tensor(kwargs, fluxes=fluxes, beam_coefs=beam_coefs)

        @staticmethod
        def backward(ctx, grad_output):
            fluxes, beam_coefs = ctx.saved_tensors
            wrt = tuple(n for n, need in zip(("fluxes", "beam_coefs"), ctx.needs_input_grad[:2]) if need)
            if not wrt:
                return None, None, None
            got = dict(zip(wrt, simulate_vis_basis_adjoint(grad_output, fluxes=fluxes, beam_coefs=beam_coefs, wrt=wrt,
                                                           **ctx.kwargs)))
            return (_as_grad(got.get("fluxes"), grad_output.device, ctx.flux_dtype),
                    _as_grad(got.get("beam_coefs"), ctx.coef_device, ctx.coef_dtype), None)

        @staticmethod
        def jvp(ctx, d_fluxes, d_beam_coefs, *_):
            fluxes, beam_coefs = ctx.saved_tensors
            if d_fluxes is None and d_beam_coefs is None:
                return None
            dv = simulate_vis_basis_jvp(fluxes=fluxes, beam_coefs=beam_coefs,
                                        **_detached(d_beam_coefs=d_beam_coefs, d_fluxes=d_fluxes), **ctx.kwargs)
            return _tangent_tensor(dv, fluxes)

    return _SimulateVisBasis


def torch_simulate_vis_basis(fluxes, beam_coefs, **kwargs):
    """The basis-beam simulation ``simulate_vis(fluxes=, beam_coefs=, beam=<K basis beams>, polarized=True, ...)`` as a torch
    operation differentiable in both tensors: ``fluxes`` real, (nsrc, nfreqs) or (nsrc, nfreqs, 4); ``beam_coefs`` complex,
    (nant, nbasis, nfreqs).  Every other argument is a keyword of ``simulate_vis``.  Returns the visibilities as a complex
    tensor on ``fluxes``' device.  The backward pass is ``simulate_vis_basis_adjoint`` of the incoming gradient, with only
    the gradients autograd asks for (``ctx.needs_input_grad``): Re(A^H g) for the real fluxes, and for the complex
    coefficients torch's convention for a complex leaf, dL = Re sum conj(grad) dC.  Forward-mode differentiation
    (``torch.autograd.forward_ad``) goes through the operation's ``jvp``: ``simulate_vis_basis_jvp`` on the tangents
    present, a missing one skipping its part."""
    return _function(_basis_autograd_function).apply(fluxes, beam_coefs, kwargs)


def _basis_array_autograd_function():
    import torch

    class _SimulateVisBasisArray(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, beam_coefs, antpos, antnums, kwargs):
            ctx.kwargs = kwargs
            ctx.antnums = antnums
            ctx.flux_dtype, ctx.coef_dtype, ctx.pos_dtype = fluxes.dtype, beam_coefs.dtype, antpos.dtype
            ctx.coef_device, ctx.pos_device = beam_coefs.device, antpos.device
            ctx.save_for_backward(fluxes, beam_coefs, antpos)
            ctx.save_for_forward(fluxes, beam_coefs, antpos)
            return _forward_tensor(dict(kwargs, ants=_ants_of(antnums, antpos)), fluxes=fluxes, beam_coefs=beam_coefs)

        @staticmethod
        def backward(ctx, grad_output):
            fluxes, beam_coefs, antpos = ctx.saved_tensors
            wrt = tuple(n for n, need in zip(("fluxes", "beam_coefs", "ants"), ctx.needs_input_grad[:3]) if need)
            if not wrt:
                return None, None, None, None, None
            got = dict(zip(wrt, simulate_vis_basis_adjoint(grad_output, ants=_ants_of(ctx.antnums, antpos), fluxes=fluxes,
                                                           beam_coefs=beam_coefs, wrt=wrt, **ctx.kwargs)))
            return (_as_grad(got.get("fluxes"), grad_output.device, ctx.flux_dtype),
                    _as_grad(got.get("beam_coefs"), ctx.coef_device, ctx.coef_dtype),
                    _as_grad(got.get("ants"), ctx.pos_device, ctx.pos_dtype), None, None)

        @staticmethod
        def jvp(ctx, d_fluxes, d_beam_coefs, d_antpos, *_):
            fluxes, beam_coefs, antpos = ctx.saved_tensors
            if d_fluxes is None and d_beam_coefs is None and d_antpos is None:
                return None
            dv = simulate_vis_basis_jvp(ants=_ants_of(ctx.antnums, antpos), fluxes=fluxes, beam_coefs=beam_coefs,
                                        **_detached(d_beam_coefs=d_beam_coefs, d_fluxes=d_fluxes, d_ants=d_antpos),
                                        **ctx.kwargs)
            return _tangent_tensor(dv, fluxes)

    return _SimulateVisBasisArray


def torch_simulate_vis_basis_array(fluxes, beam_coefs, antpos, *, antnums=None, **kwargs):
    """The basis-beam simulation as a torch operation differentiable in the fluxes, the coefficients and the antenna
    positions -- the three unknowns of a joint beam and array fit: ``fluxes`` real, (nsrc, nfreqs) or (nsrc, nfreqs, 4);
    ``beam_coefs`` complex, (nant, nbasis, nfreqs); ``antpos`` real, (nant, 3), ENU metres.  ``antnums`` gives the
    dictionary keys ``baselines`` refers to (default ``range(nant)``); every other argument is a keyword of
    ``simulate_vis`` -- but for ``ants``, which ``antpos`` replaces (TypeError).  Returns the visibilities as a complex
    tensor on ``fluxes``' device.  The backward pass is one ``simulate_vis_basis_adjoint`` call with only the gradients
    autograd asks for (``ctx.needs_input_grad``); forward mode (``torch.autograd.forward_ad``) runs
    ``simulate_vis_basis_jvp`` on the tangents present."""
    antnums = _checked_antnums("torch_simulate_vis_basis_array", antpos, antnums, kwargs)
    return _function(_basis_array_autograd_function).apply(fluxes, beam_coefs, antpos, antnums, kwargs)


# device bytes of one call's (ndir, ...) output: longer stacks of directions are cut into groups under it
BASIS_TANGENT_BYTES_ENV = "FFTVIS_BASIS_TANGENT_BYTES"
BASIS_TANGENT_BYTES_DEFAULT = 1 << 30


def simulate_vis_basis_jvp(
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    beam_coefs,
    telescope_loc,
    *,
    d_beam_coefs=None,
    d_fluxes=None,
    d_ants=None,
    d_baselines=None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = True,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Forward-mode tangent (Jacobian-vector product) of the basis-beam simulation ``simulate_vis(..., beam=<K basis
    beams>, beam_coefs=C)`` along directions of the coefficients, of the fluxes and of the antenna positions,

        dV = dV[C; d_beam_coefs]  +  dV/d(fluxes) . d_fluxes  +  dV/d(ants) . d_ants,
        dV_b[C; D] = sum_kl ( conj(D[a1,k]) C[a2,l] + conj(C[a1,k]) D[a2,l] ) M_kl(b),

    M_kl the visibilities of basis beams k and l.  They depend on neither C nor D, so the coefficient part is one forward
    run whose gather carries the differentiated weights (``fv_sim_run_basis_tangent``), and any number of directions share
    its transforms.  It is the transpose of ``simulate_vis_basis_adjoint``: for every G,
    ``Re <dV, G> = Re <d_beam_coefs, gcoefs> + <d_fluxes, gflux> + d_baselines . gbls``.

    * ``d_beam_coefs``: complex, (nant, nbasis, nfreqs) -- the result has ``simulate_vis``'s shape and dtype -- or a stack
      (ndir, nant, nbasis, nfreqs) -- the result gains a leading ``ndir`` axis, direction q equal, bit for bit, to the call
      on ``d_beam_coefs[q]`` alone.  A long stack is cut into groups whose device output stays under
      ``FFTVIS_BASIS_TANGENT_BYTES`` (default 1 GiB); every group is one forward run.
    * ``d_fluxes``: ``fluxes``' shape.  The map is linear in the fluxes, so this part is one ``simulate_vis(...,
      beam_coefs=C)`` run on ``d_fluxes``, added to the rest.  It combines with an unbatched ``d_beam_coefs`` only: with a
      stack it is a ValueError (flux directions are plain forward runs).
    * ``d_ants``: (nant, 3), ENU metres, rows in ``ants``' iteration order, turned into ``d_baselines`` on the host
      (``antenna_to_baseline_tangent``); ``d_baselines``: (nbls, 3), every listed baseline an independent vector.  Giving
      both is a ValueError.  The part is ``sum_d i (2 pi nu / c) d_baselines[k, d] D_d`` with D_d the basis simulation of the
      fluxes times topo_d (``fv_sim_run_basis_position_tangent``: about three forward runs), added to the rest; on a flat
      array the up component still enters.  With a stack of ``d_beam_coefs`` it is a ValueError.

    The source positions have a pass of their own, ``simulate_vis_basis_source_jvp``.  Not covered: a lattice form, several
    position directions per call.

    No input at all gives zeros.  numpy arrays, or torch tensors: when a tangent is a tensor on the run's device
    ``d_beam_coefs`` is handed over by pointer and the result is a tensor on that device; host tensors in, a host tensor
    out.  Every other keyword means what it means for ``simulate_vis``, ``reference_compat`` included.  ``polarized`` must
    be True and ``beam_idx`` None, as for the forward."""
    import os

    args = locals()
    if beam_coefs is None:
        raise ValueError("simulate_vis_basis_jvp needs beam_coefs (simulate_vis_jvp covers per-antenna beam_idx)")
    if not polarized:  # the forward's message
        raise ValueError(
            "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
        )
    run = _describe_run(args)
    c_shape = run.beam_coefs.shape
    fluxes = _host_fluxes(run, fluxes, d_fluxes)
    stacked = False
    if d_beam_coefs is not None:
        dshape = tuple(d_beam_coefs.shape)
        if dshape != c_shape and not (len(dshape) == 4 and dshape[0] >= 1 and dshape[1:] == c_shape):
            raise ValueError(f"d_beam_coefs must have beam_coefs' shape {c_shape} or (ndir,) + that shape, got {dshape}")
        stacked = len(dshape) == 4
        if not (np.iscomplexobj(d_beam_coefs) if not _is_tensor(d_beam_coefs) else d_beam_coefs.is_complex()):
            raise ValueError("d_beam_coefs must be complex, like beam_coefs")
        if stacked and d_fluxes is not None:
            raise ValueError("d_fluxes combines with one direction of the coefficients only, not with a stack "
                             "(flux directions are plain simulate_vis runs)")
        if stacked and (d_ants is not None or d_baselines is not None):
            raise ValueError("a position tangent (d_ants / d_baselines) combines with one direction of the coefficients "
                             "only, not with a stack")
    tangents = (d_beam_coefs, d_fluxes, d_ants, d_baselines)
    d_baselines = _baseline_tangent(run, d_ants, d_baselines)
    try:
        budget = float(os.environ.get(BASIS_TANGENT_BYTES_ENV, BASIS_TANGENT_BYTES_DEFAULT))
    except ValueError:
        raise ValueError(f"{BASIS_TANGENT_BYTES_ENV} must be a number of bytes") from None
    device = _run_device(run, tangents, "a tangent")
    ndir = int(d_beam_coefs.shape[0]) if stacked else 1
    dv = _zeros(device, (ndir,) + run.vis_shape, run.cdt)
    dd = _buffer(run, device, d_beam_coefs, "complex")
    if dd is not None:
        dd = dd.reshape((ndir,) + c_shape)
        _synchronize(device)
        per_dir = int(np.prod(run.vis_shape)) * np.dtype(run.cdt).itemsize
        group = int(max(1, min(ndir, budget // max(per_dir, 1))))
        for q0 in range(0, ndir, group):
            q1 = min(ndir, q0 + group)
            _engine_simulate(run, fluxes, basis_tangent_of=(dd[q0:q1], dv[q0:q1]))
    if d_baselines is not None:
        db = _buffer(run, device, d_baselines, "float64")
        dp = _zeros(device, run.vis_shape, run.cdt)
        _synchronize(device)
        dv[0] += _engine_simulate(run, fluxes, tangent_of=(db, None, dp))
    if d_fluxes is not None:
        _forward_simulate(run, d_fluxes, dv[0])
    if not stacked:
        dv = dv[0]
    if device is None and any(_is_tensor(x) for x in tangents):  # host tensors in, a host tensor out
        import torch

        dv = torch.from_numpy(np.ascontiguousarray(dv))
    return dv


def baseline_to_antenna_gradient(gbls, ants: dict, baselines: list):
    """Scatter a gradient with respect to the baseline vectors, ``gbls`` (nbls, 3), to the antennas: baseline (i, j) is
    ``ants[j] - ants[i]``, so row j receives ``+gbls[k]`` and row i ``-gbls[k]``.  Returns (nant, 3) with rows in
    ``ants``' iteration order, numpy for numpy input and a tensor on ``gbls``' device for a tensor.  An auto-correlation
    contributes nothing, and the rows sum to zero: a common shift of the array changes no visibility."""
    row = {a: i for i, a in enumerate(ants)}
    i0 = np.array([row[b[0]] for b in baselines], dtype=np.int64)
    i1 = np.array([row[b[1]] for b in baselines], dtype=np.int64)
    if tuple(gbls.shape) != (len(baselines), 3):
        raise ValueError(f"gbls must have shape ({len(baselines)}, 3), got {tuple(gbls.shape)}")
    if _is_tensor(gbls):
        import torch

        out = torch.zeros((len(row), 3), dtype=gbls.dtype, device=gbls.device)
        out.index_add_(0, torch.as_tensor(i1, device=gbls.device), gbls)
        out.index_add_(0, torch.as_tensor(i0, device=gbls.device), -gbls)
        return out
    out = np.zeros((len(row), 3), dtype=np.float64)
    np.add.at(out, i1, gbls)
    np.subtract.at(out, i0, gbls)
    return out


def simulate_vis_position_adjoint(
    vis,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    wrt="ants",
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    beam_coefs: np.ndarray = None,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Gradient of ``simulate_vis(ants, fluxes, ...)`` with respect to the antenna positions, for a visibility-shaped
    ``vis`` (G = dL/dV, dL = Re sum conj(G) dV), in ENU metres^-1.

    Every path of the simulation approximates V_k = cj_k(sum_j c_j exp(2 pi i nu s_k b_k . topo_j / c)),
    b_k = ants[j] - ants[i]; the strengths c do not depend on the positions, so dV_k / db_k,d = i (2 pi nu / c) D_d with D_d
    the simulation of the fluxes times topo_d, and
    ``gbls[k, d] = -sum_{f,t,r} (2 pi nu_f / c) Im(conj(G) D_d)``: the gradient of the smooth exact map.  Which path the
    forward takes is a piecewise decision and does not enter; on a coplanar array, where the forward drops the heights,
    the up component is still returned (someone fitting antenna heights starts from a flat model).

    * ``wrt="baselines"``: (nbls, 3) float64, every listed baseline an independent vector;
    * ``wrt="ants"``: (nant, 3) float64, rows in ``ants``' iteration order: ``baseline_to_antenna_gradient`` of the
      baseline result, formed on the host;
    * a tuple of both names returns a tuple in that order.

    ``fluxes`` is the forward's, (nsrc, nfreqs) or (nsrc, nfreqs, 4).  ``vis`` is a numpy array or a torch tensor on the
    run's device (handed over by pointer; the results are then tensors on that device).  Every other keyword means what it
    means for ``simulate_vis``, ``reference_compat`` included; ``force_use_type3`` is accepted and always on: the pass runs
    the type-3 transform (about three forward runs whatever the number of antennas), so an ideal lattice array works and
    takes its redundant runs.  Not covered: ``beam_coefs`` (NotImplementedError; ``simulate_vis_basis_adjoint`` has
    ``wrt="ants"``), a type-1 (lattice) form of the pass."""
    args = locals()
    single, names = _parse_wrt(wrt, ("ants", "baselines"), "'ants', 'baselines' or both")
    if beam_coefs is not None:
        raise NotImplementedError("simulate_vis_position_adjoint does not support basis beams (beam_coefs): "
                                  "simulate_vis_basis_adjoint(wrt='ants') does")
    run = _describe_run(args)
    fluxes = _host_fluxes(run, fluxes)
    g, (gbls,), on_device = _gradient_buffers(run, vis, [((run.nbls, 3), "float64")])
    gbls = _engine_simulate(run, fluxes, force_use_type3=True, adjoint_of=(g, gbls), adjoint_wrt="positions")
    res = {"baselines": gbls}
    if "ants" in names:
        res["ants"] = baseline_to_antenna_gradient(gbls, run.ants, run.baselines)
    return _select(res, single, names, vis, on_device)


def _tangent_tensor(dv, like):
    """A tangent of ``simulate_vis_jvp`` as a tensor on the device of the operation's output (``like``: the fluxes)."""
    import torch

    if not _is_tensor(dv):
        dv = torch.from_numpy(np.ascontiguousarray(dv))
    return dv.to(like.device)


def _array_autograd_function():
    import torch

    class _SimulateVisArray(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, antpos, antnums, kwargs):
            ctx.kwargs = kwargs
            ctx.antnums = antnums
            ctx.full_stokes = fluxes.ndim == 3
            ctx.flux_dtype, ctx.pos_dtype, ctx.pos_device = fluxes.dtype, antpos.dtype, antpos.device
            ctx.save_for_backward(fluxes, antpos)
            ctx.save_for_forward(fluxes, antpos)
            return _forward_tensor(dict(kwargs, ants=_ants_of(antnums, antpos)), fluxes=fluxes)

        @staticmethod
        def backward(ctx, grad_output):
            fluxes, antpos = ctx.saved_tensors
            ants = _ants_of(ctx.antnums, antpos)
            gf = gp = None
            if ctx.needs_input_grad[0]:
                gf = simulate_vis_adjoint(grad_output, ants=ants, full_stokes=ctx.full_stokes, **ctx.kwargs)
            if ctx.needs_input_grad[1]:
                gp = simulate_vis_position_adjoint(grad_output, ants=ants, fluxes=fluxes, wrt="ants", **ctx.kwargs)
            return (_as_grad(gf, grad_output.device, ctx.flux_dtype), _as_grad(gp, ctx.pos_device, ctx.pos_dtype),
                    None, None)

        @staticmethod
        def jvp(ctx, d_fluxes, d_antpos, *_):
            fluxes, antpos = ctx.saved_tensors
            if d_fluxes is None and d_antpos is None:
                return None
            dv = simulate_vis_jvp(ants=_ants_of(ctx.antnums, antpos), fluxes=fluxes,
                                  **_detached(d_ants=d_antpos, d_fluxes=d_fluxes), **ctx.kwargs)
            return _tangent_tensor(dv, fluxes)

    return _SimulateVisArray


def torch_simulate_vis_array(fluxes, antpos, *, antnums=None, **kwargs):
    """``simulate_vis`` as a torch operation differentiable in the fluxes and in the antenna positions: ``fluxes`` real,
    (nsrc, nfreqs) or (nsrc, nfreqs, 4); ``antpos`` real, (nant, 3), ENU metres.  ``antnums`` gives the dictionary keys
    ``baselines`` refers to (default ``range(nant)``); every other argument is a keyword of ``simulate_vis`` -- but for
    ``ants``, which the two tensors replace (TypeError).  Returns the visibilities as a complex tensor on ``fluxes``'
    device.  The backward pass runs only what autograd asks for (``ctx.needs_input_grad``): ``simulate_vis_adjoint`` for
    the fluxes, ``simulate_vis_position_adjoint`` for the positions.  Forward mode (``torch.autograd.forward_ad``) runs
    ``simulate_vis_jvp`` on the tangents present."""
    antnums = _checked_antnums("torch_simulate_vis_array", antpos, antnums, kwargs)
    if kwargs.get("beam_coefs") is not None:
        raise NotImplementedError("torch_simulate_vis_array does not support basis beams (beam_coefs): "
                                  "torch_simulate_vis_basis_array does")
    return _function(_array_autograd_function).apply(fluxes, antpos, antnums, kwargs)


# Angular step [rad] of the central differences that give d n(t) / d(ra, dec) under device astrometry (``radec_jacobian``):
# the chain is smooth on the scale of a radian, so the truncation is about h^2 / 6 = 2e-11 and the rounding of the fp64
# vectors about 1e-16 / h = 1e-11, both relative.
ASTROM_JACOBIAN_STEP = 1e-5


def radec_jacobian(ra, dec, times, telescope_loc, *, astrom=None, device: int = 0) -> np.ndarray:
    """J[t, j] = d n_j(t) / d(ra_j, dec_j), (ntimes, nsrc, 3, 2) float64: the derivative of the topocentric (east, north,
    up) unit vectors the simulation uses with respect to the catalog's angles.  Without ``astrom`` the chain is
    ``coord_method="SiderealRotation"``'s, n = R_t eq(ra, dec), in closed form.  With ``astrom`` ((ntimes, 31) contexts,
    device astrometry) it is taken by central differences of ``gpu.utils.astrom_topo`` (the device's own chain, in fp64)
    at the fixed angular step ``ASTROM_JACOBIAN_STEP``, along unit-speed great circles: towards increasing declination,
    and along the tangent of the parallel (times cos dec)."""
    ra = np.asarray(ra, dtype=np.float64).ravel()
    dec = np.asarray(dec, dtype=np.float64).ravel()
    sr, cr, sd, cd = np.sin(ra), np.cos(ra), np.sin(dec), np.cos(dec)
    d_ra = np.stack([-cd * sr, cd * cr, np.zeros_like(ra)])   # d eq / d ra   (3, nsrc)
    d_dec = np.stack([-sd * cr, -sd * sr, cd])                # d eq / d dec
    if astrom is None:
        from .core.coords import SiderealRotation

        R = SiderealRotation(times, telescope_loc).matrices()  # (ntimes, 3, 3)
        return np.stack([np.einsum("tab,bj->tja", R, d_ra), np.einsum("tab,bj->tja", R, d_dec)], axis=-1)
    from .core.coords import eq_unit_vectors
    from .gpu.utils import astrom_topo

    astrom = np.ascontiguousarray(astrom, dtype=np.float64)
    if astrom.ndim != 2 or astrom.shape[1] != 31:
        raise ValueError("astrom must have shape (ntimes, 31): one eraASTROM context per time")
    eq = eq_unit_vectors(ra, dec)
    h = ASTROM_JACOBIAN_STEP
    e_ra = np.stack([-sr, cr, np.zeros_like(ra)])  # unit tangent of the parallel: d eq / d ra = cos(dec) e_ra
    out = np.empty((astrom.shape[0], ra.size, 3, 2))
    for t, ctx in enumerate(astrom):
        for c, (e, scale) in enumerate(((e_ra, cd), (d_dec, 1.0))):
            plus = astrom_topo(np.cos(h) * eq + np.sin(h) * e, ctx, device)
            minus = astrom_topo(np.cos(h) * eq - np.sin(h) * e, ctx, device)
            out[t, :, :, c] = ((plus - minus) / (2.0 * h) * scale).T
    return out


def topo_to_radec_gradient(gtopo, jacobian):
    """Chain a gradient with respect to the topocentric unit vectors, ``gtopo`` (ntimes, nsrc, 3), to the catalog's angles:
    ``sum_t J_t^T gtopo[t]`` with ``jacobian`` = J (ntimes, nsrc, 3, 2) from ``radec_jacobian``.  Returns (nsrc, 2), columns
    (ra, dec), numpy for numpy input and a tensor on ``gtopo``'s device for a tensor."""
    if len(gtopo.shape) != 3 or gtopo.shape[2] != 3 or tuple(jacobian.shape) != tuple(gtopo.shape) + (2,):
        raise ValueError(f"gtopo must be (ntimes, nsrc, 3) and jacobian (ntimes, nsrc, 3, 2), got {tuple(gtopo.shape)} and "
                         f"{tuple(jacobian.shape)}")
    if _is_tensor(gtopo):
        import torch

        J = torch.as_tensor(np.asarray(jacobian) if not _is_tensor(jacobian) else jacobian, dtype=gtopo.dtype, device=gtopo.device)
        return torch.einsum("tjd,tjdc->jc", gtopo, J)
    return np.einsum("tjd,tjdc->jc", np.asarray(gtopo, dtype=np.float64), np.asarray(jacobian, dtype=np.float64))


def simulate_vis_source_adjoint(
    vis,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    wrt="radec",
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    beam_coefs: np.ndarray = None,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Gradient of ``simulate_vis(ants, fluxes, ra, dec, ...)`` with respect to the source positions, for a
    visibility-shaped ``vis`` (G = dL/dV, dL = Re sum conj(G) dV).

    Every path of the simulation approximates V_k = cj_k(sum_j c_j(n_j) exp(2 pi i nu s_k b_k . n_j / c)), n_j(t) the
    source's topocentric (east, north, up) unit vector and c the apparent strengths, which depend on n through the beams.
    The gradient has a phase term (transforms of the adjoint's strengths times the baseline coordinates) and a beam term
    (central differences of the beams at a fixed angular step, with the transform's values held fixed): the gradient of the
    smooth exact map, whichever path the forward takes.  The horizon cut is a piecewise decision and is not differentiated:
    a source below the horizon at time t contributes exactly 0 at that t.

    * ``wrt="topo"``: (ntimes, nsrc, 3) float64, ENU, tangential (n . g = 0): dL = sum g[t, j] . delta_j(t) for small
      displacements delta perpendicular to n.  Valid with every source of coordinates -- rotation matrices, ``coord_mgr=``,
      ``astrom=`` / ``device_astrometry=True``;
    * ``wrt="radec"``: (nsrc, 2) float64, columns (ra, dec), per radian: ``topo_to_radec_gradient`` of the above with
      ``radec_jacobian`` -- closed form for ``coord_method="SiderealRotation"``, central differences of the device's own
      chain under device astrometry.  With a caller's ``coord_mgr`` (or a matvis manager the engine would build) the chain
      from (ra, dec) to the vectors is not this package's: ValueError, ask for ``wrt="topo"`` and chain it yourself;
    * a tuple of both names returns a tuple in that order.

    ``fluxes`` is the forward's, (nsrc, nfreqs) or (nsrc, nfreqs, 4).  ``vis`` is a numpy array or a torch tensor on the
    run's device (handed over by pointer; the results are then tensors on that device).  Every other keyword means what it
    means for ``simulate_vis``, ``reference_compat`` included; ``force_use_type3`` is accepted and always on: the pass runs
    the type-3 transform -- 1 + D transforms where the flux adjoint runs one, D = 2 on a flat array and 3 otherwise -- so an
    ideal lattice array works through it.  Not covered: ``beam_coefs`` (NotImplementedError)."""
    args = locals()
    single, names = _parse_wrt(wrt, ("topo", "radec"), "'topo', 'radec' or both")
    if beam_coefs is not None:
        raise NotImplementedError("simulate_vis_source_adjoint does not support basis beams (beam_coefs)")
    run = _describe_run(args)
    run = _own_radec_chain(run, "wrt='radec'", "radec" in names, "ask for wrt='topo' and apply its Jacobian",
                           "ask for wrt='topo'")
    fluxes = _host_fluxes(run, fluxes)
    g, (gtopo,), on_device = _gradient_buffers(run, vis, [((run.ntimes, run.nsrc, 3), "float64")])
    gtopo = _engine_simulate(run, fluxes, force_use_type3=True, adjoint_of=(g, gtopo), adjoint_wrt="sources")
    res = {"topo": gtopo}
    if "radec" in names:
        res["radec"] = topo_to_radec_gradient(gtopo, _radec_jacobian_of(run))
    return _select(res, single, names, vis, on_device)


def antenna_to_baseline_tangent(d_ants, ants: dict, baselines: list):
    """The change of the baseline vectors along a change ``d_ants`` (nant, 3) of the antenna positions, rows in ``ants``'
    iteration order: baseline (i, j) is ``ants[j] - ants[i]``, so row k is ``d_ants[j_k] - d_ants[i_k]`` -- the transpose
    of ``baseline_to_antenna_gradient``.  Returns (nbls, 3), numpy for numpy input and a tensor on ``d_ants``' device
    for a tensor."""
    row = {a: i for i, a in enumerate(ants)}
    i0 = np.array([row[b[0]] for b in baselines], dtype=np.int64)
    i1 = np.array([row[b[1]] for b in baselines], dtype=np.int64)
    if tuple(d_ants.shape) != (len(row), 3):
        raise ValueError(f"d_ants must have shape ({len(row)}, 3), got {tuple(d_ants.shape)}")
    if _is_tensor(d_ants):
        import torch

        return d_ants[torch.as_tensor(i1, device=d_ants.device)] - d_ants[torch.as_tensor(i0, device=d_ants.device)]
    d_ants = np.asarray(d_ants, dtype=np.float64)
    return d_ants[i1] - d_ants[i0]


def simulate_vis_jvp(
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    d_ants=None,
    d_baselines=None,
    d_radec=None,
    d_topo=None,
    d_fluxes=None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    beam_coefs: np.ndarray = None,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Forward-mode tangent (Jacobian-vector product) of ``simulate_vis(ants, fluxes, ra, dec, ...)``: the change dV of the
    visibilities along a direction of the parameters, an array of ``simulate_vis``'s shape and dtype,

        dV = dV/d(ants) . d_ants  +  dV/d(positions of the sources) . d_radec  +  dV/d(fluxes) . d_fluxes.

    Both position derivatives of the exact sum every forward path approximates are forward transforms of other strengths
    (``fv_sim_run_tangent``): about three forward runs for the antennas and 1 + D for the sources (D = 2 on a flat array,
    3 otherwise), whatever the number of parameters.  It is the transpose of the adjoints: for every G,
    ``Re <dV, G> = d_baselines . gbls + d_topo . gtopo + d_fluxes . gflux`` with the gradients of
    ``simulate_vis_position_adjoint``, ``simulate_vis_source_adjoint`` and ``simulate_vis_adjoint``.

    * ``d_ants``: (nant, 3), ENU metres, rows in ``ants``' iteration order; ``d_baselines[k] = d_ants[j_k] - d_ants[i_k]``
      is formed on the host (``antenna_to_baseline_tangent``).  ``d_baselines``: (nbls, 3), every listed baseline an
      independent vector.  Giving both is a ValueError.  On a flat array the up component still enters.
    * ``d_radec``: (nsrc, 2) radians, columns (ra, dec), chained on the host through ``radec_jacobian`` -- for
      ``coord_method="SiderealRotation"`` and device astrometry; with a caller's ``coord_mgr`` (or a matvis manager the
      engine would build) only ``d_topo`` is served: ValueError.  ``d_topo``: (ntimes, nsrc, 3), ENU; its radial part is
      removed (the directions are unit vectors), and a source below the horizon at time t contributes exactly 0 there.
      Giving both is a ValueError.
    * ``d_fluxes``: ``fluxes``' shape.  The map is linear in the fluxes, so this part is one ``simulate_vis`` run on
      ``d_fluxes``, added to the rest.

    No input at all gives zeros.  numpy arrays, or torch tensors: when any of the tangents is a tensor on the run's device
    the position tangents are handed over by pointer and the result is a tensor on that device; host tensors in, a host
    tensor out.  Every other keyword means what it means for ``simulate_vis``, ``reference_compat`` included;
    ``force_use_type3`` is accepted and always on for the position parts: the pass runs the type-3 transform.  Not
    covered: ``beam_coefs`` (NotImplementedError; ``simulate_vis_basis_jvp`` takes ``d_ants`` / ``d_baselines``), a type-1
    (lattice) form of the pass."""
    args = locals()
    if beam_coefs is not None:
        raise NotImplementedError("simulate_vis_jvp does not support basis beams (beam_coefs): "
                                  "simulate_vis_basis_jvp(d_ants=) does")
    if d_radec is not None and d_topo is not None:
        raise ValueError("give the source tangent as d_radec or as d_topo, not both")
    run = _describe_run(args)
    run = _own_radec_chain(run, "d_radec", d_radec is not None, "apply its Jacobian and pass d_topo", "pass d_topo")
    tangents = (d_ants, d_baselines, d_radec, d_topo, d_fluxes)
    device = _run_device(run, tangents, "a tangent")
    fluxes = _host_fluxes(run, fluxes, d_fluxes)
    d_baselines = _baseline_tangent(run, d_ants, d_baselines)
    if d_radec is not None and tuple(d_radec.shape) != (run.nsrc, 2):
        raise ValueError(f"d_radec must have shape ({run.nsrc}, 2), got {tuple(d_radec.shape)}")
    if d_topo is not None and tuple(d_topo.shape) != (run.ntimes, run.nsrc, 3):
        raise ValueError(f"d_topo must have shape ({run.ntimes}, {run.nsrc}, 3), got {tuple(d_topo.shape)}")
    if d_radec is not None:
        d_topo = np.einsum("tjdc,jc->tjd", _radec_jacobian_of(run), _host(d_radec).astype(np.float64))
    db, dt_ = _buffer(run, device, d_baselines, "float64"), _buffer(run, device, d_topo, "float64")
    dv = _zeros(device, run.vis_shape, run.cdt)
    if db is not None or dt_ is not None:
        _synchronize(device)
        dv = _engine_simulate(run, fluxes, force_use_type3=True, tangent_of=(db, dt_, dv))
    if d_fluxes is not None:
        _forward_simulate(run, d_fluxes, dv)
    if device is None and any(_is_tensor(x) for x in tangents):  # host tensors in, a host tensor out
        import torch

        dv = torch.from_numpy(np.ascontiguousarray(dv))
    return dv


def _radec_columns(radec) -> dict:
    rd = radec.detach().cpu().numpy().astype(np.float64)
    return dict(ra=rd[:, 0].copy(), dec=rd[:, 1].copy())


def _sky_autograd_function():
    import torch

    class _SimulateVisSky(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, radec, kwargs):
            ctx.kwargs = kwargs
            ctx.full_stokes = fluxes.ndim == 3
            ctx.flux_dtype, ctx.pos_dtype, ctx.pos_device = fluxes.dtype, radec.dtype, radec.device
            ctx.save_for_backward(fluxes, radec)
            ctx.save_for_forward(fluxes, radec)
            return _forward_tensor(dict(kwargs, **_radec_columns(radec)), fluxes=fluxes)

        @staticmethod
        def backward(ctx, grad_output):
            fluxes, radec = ctx.saved_tensors
            pos = _radec_columns(radec)
            gf = gp = None
            if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:  # one pass for both
                gf, gp = simulate_vis_sky_adjoint(grad_output, fluxes=fluxes, wrt=("fluxes", "radec"), **pos, **ctx.kwargs)
            elif ctx.needs_input_grad[0]:
                gf = simulate_vis_adjoint(grad_output, full_stokes=ctx.full_stokes, **pos, **ctx.kwargs)
            elif ctx.needs_input_grad[1]:
                gp = simulate_vis_source_adjoint(grad_output, fluxes=fluxes, wrt="radec", **pos, **ctx.kwargs)
            return _as_grad(gf, grad_output.device, ctx.flux_dtype), _as_grad(gp, ctx.pos_device, ctx.pos_dtype), None

        @staticmethod
        def jvp(ctx, d_fluxes, d_radec, _):
            fluxes, radec = ctx.saved_tensors
            if d_fluxes is None and d_radec is None:
                return None
            dv = simulate_vis_jvp(fluxes=fluxes, **_radec_columns(radec),
                                  **_detached(d_radec=d_radec, d_fluxes=d_fluxes), **ctx.kwargs)
            return _tangent_tensor(dv, fluxes)

    return _SimulateVisSky


def torch_simulate_vis_sky(fluxes, radec, **kwargs):
    """``simulate_vis`` as a torch operation differentiable in the fluxes and in the source positions: ``fluxes`` real,
    (nsrc, nfreqs) or (nsrc, nfreqs, 4); ``radec`` real, (nsrc, 2), columns (ra, dec) in radians.  Every other argument is a
    keyword of ``simulate_vis`` -- but for ``ra`` and ``dec``, which the tensor replaces (TypeError).  Returns the
    visibilities as a complex tensor on ``fluxes``' device.  The backward pass runs only what autograd asks for
    (``ctx.needs_input_grad``): ``simulate_vis_adjoint`` for the fluxes, ``simulate_vis_source_adjoint(wrt="radec")`` for the
    positions, which needs ``coord_method="SiderealRotation"`` or device astrometry, and when both are asked for one
    ``simulate_vis_sky_adjoint`` call, whose pass shares the transforms.  Forward mode
    (``torch.autograd.forward_ad``) runs ``simulate_vis_jvp`` on the tangents present, under the same condition."""
    if "ra" in kwargs or "dec" in kwargs:
        raise TypeError("torch_simulate_vis_sky takes the source positions as the tensor radec, not ra= / dec=")
    if kwargs.get("beam_coefs") is not None:
        raise NotImplementedError("torch_simulate_vis_sky does not support basis beams (beam_coefs)")
    if "adjoint_path" in kwargs:
        raise TypeError("torch_simulate_vis_sky does not take adjoint_path: its passes run the type-3 transform")
    if radec.ndim != 2 or radec.shape[1] != 2 or radec.is_complex():
        raise ValueError(f"radec must be a real (nsrc, 2) tensor, got {tuple(radec.shape)} {radec.dtype}")
    return _function(_sky_autograd_function).apply(fluxes, radec, kwargs)


def _basis_run(name, args) -> _Run:
    """The run of a source pass through basis beams: the forward's refusals first."""
    if args["beam_coefs"] is None:
        raise ValueError(f"{name} needs beam_coefs (without basis beams simulate_vis_source_adjoint and simulate_vis_jvp "
                         "are the passes)")
    if not args["polarized"]:  # the forward's message
        raise ValueError(
            "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
        )
    return _describe_run(args)


def simulate_vis_basis_source_adjoint(
    vis,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    beam_coefs,
    telescope_loc,
    *,
    wrt="radec",
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = True,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Gradient of the basis-beam simulation ``simulate_vis(..., beam=<K basis beams>, beam_coefs=C)`` with respect to the
    source positions, for a visibility-shaped ``vis`` (G = dL/dV, dL = Re sum conj(G) dV): ``simulate_vis_source_adjoint``'s
    quantity through basis beams.

    V_b = sum_{k<=l} (w1 M_kl(b) + w2 M_kl(b) at the feed-transposed slot), w1 = conj(C[a1,k]) C[a2,l],
    w2 = conj(C[a1,l]) C[a2,k] (``reference_compat=False``: the (l, k) part of an off-diagonal term of complex beams is
    conj(M_kl(-b))^T), and every M_kl is a sum over sources of the strengths of basis beams k and l times the phase: the
    gradient is the source pass's, once per term -- a phase term and a beam term, summed over the terms
    (``fv_sim_run_basis_source_adjoint``).  Tangential, exactly 0 below the horizon; the horizon cut and the path choice
    are not differentiated; between two order-0 tables the beam term is 0 by definition, decided per term.

    * ``wrt="topo"``: (ntimes, nsrc, 3) float64, ENU, tangential; valid with every source of coordinates;
    * ``wrt="radec"``: (nsrc, 2) float64, columns (ra, dec), per radian: ``topo_to_radec_gradient`` of the above with
      ``radec_jacobian`` -- for ``coord_method="SiderealRotation"`` and device astrometry; with a ``coord_mgr`` (or a matvis
      manager the engine would build) ValueError: ask for ``wrt="topo"``;
    * a tuple of both names returns a tuple in that order.

    ``fluxes`` and ``beam_coefs`` are the forward's.  ``vis`` is a numpy array or a torch tensor on the run's device
    (handed over by pointer; the results are then tensors on that device).  Every other keyword means what it means for
    ``simulate_vis``, ``reference_compat`` included; ``polarized`` must be True and ``beam_idx`` None, as for the forward.
    The cost is 1 + D transforms per term where ``simulate_vis_basis_adjoint(wrt="fluxes")`` runs one (D = 2 on a flat
    array, 3 otherwise) plus five beam evaluations per (source, channel, term).  ``simulate_vis_basis_sky_adjoint`` returns
    the flux gradient from the same transforms.  Not covered: a lattice form, several directions per call, multi-GPU."""
    args = locals()
    single, names = _parse_wrt(wrt, ("topo", "radec"), "'topo', 'radec' or both")
    run = _basis_run("simulate_vis_basis_source_adjoint", args)
    run = _own_radec_chain(run, "wrt='radec'", "radec" in names, "ask for wrt='topo' and apply its Jacobian",
                           "ask for wrt='topo'")
    fluxes = _host_fluxes(run, fluxes)
    g, (gtopo,), on_device = _gradient_buffers(run, vis, [((run.ntimes, run.nsrc, 3), "float64")])
    gtopo = _engine_simulate(run, fluxes, basis_source_of=("adjoint", g, gtopo))
    res = {"topo": gtopo}
    if "radec" in names:
        res["radec"] = topo_to_radec_gradient(gtopo, _radec_jacobian_of(run))
    return _select(res, single, names, vis, on_device)


def simulate_vis_basis_source_jvp(
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    beam_coefs,
    telescope_loc,
    *,
    d_radec=None,
    d_topo=None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = True,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Forward-mode tangent of the basis-beam simulation ``simulate_vis(..., beam=<K basis beams>, beam_coefs=C)`` along a
    change of the source positions: dV in ``simulate_vis``'s shape and dtype, the transpose of
    ``simulate_vis_basis_source_adjoint`` -- ``Re <dV, G> = sum d_topo . gtopo`` for every G.

    * ``d_radec``: (nsrc, 2) radians, columns (ra, dec), chained on the host through ``radec_jacobian`` -- for
      ``coord_method="SiderealRotation"`` and device astrometry; with a ``coord_mgr`` (or a matvis manager the engine would
      build) only ``d_topo`` is served: ValueError;
    * ``d_topo``: (ntimes, nsrc, 3), ENU; its radial part is removed, and a source below the horizon at time t contributes
      exactly 0 there.  Giving both is a ValueError.

    Per (k <= l) term the 1 + D strength sets of ``simulate_vis_jvp``'s source side with the term's beams, and 1 + D rounds
    whose gathers carry the basis weights (``fv_sim_run_basis_source_tangent``).  With neither input: zeros and no device
    work.  numpy arrays, or torch tensors: a tangent on the run's device is handed over by pointer and the result is a
    tensor on that device; host tensors in, a host tensor out.  Every other keyword means what it means for
    ``simulate_vis``.  Not covered: a lattice form, several directions per call."""
    args = locals()
    if d_radec is not None and d_topo is not None:
        raise ValueError("give the source tangent as d_radec or as d_topo, not both")
    run = _basis_run("simulate_vis_basis_source_jvp", args)
    run = _own_radec_chain(run, "d_radec", d_radec is not None, "apply its Jacobian and pass d_topo", "pass d_topo")
    tangents = (d_radec, d_topo)
    device = _run_device(run, tangents, "a tangent")
    fluxes = _host_fluxes(run, fluxes)
    if d_radec is not None and tuple(d_radec.shape) != (run.nsrc, 2):
        raise ValueError(f"d_radec must have shape ({run.nsrc}, 2), got {tuple(d_radec.shape)}")
    if d_topo is not None and tuple(d_topo.shape) != (run.ntimes, run.nsrc, 3):
        raise ValueError(f"d_topo must have shape ({run.ntimes}, {run.nsrc}, 3), got {tuple(d_topo.shape)}")
    if d_radec is not None:
        d_topo = np.einsum("tjdc,jc->tjd", _radec_jacobian_of(run), _host(d_radec).astype(np.float64))
    dt_ = _buffer(run, device, d_topo, "float64")
    dv = _zeros(device, run.vis_shape, run.cdt)
    if dt_ is not None:
        _synchronize(device)
        dv = _engine_simulate(run, fluxes, basis_source_of=("tangent", dt_, dv))
    if device is None and any(_is_tensor(x) for x in tangents):  # host tensors in, a host tensor out
        import torch

        dv = torch.from_numpy(np.ascontiguousarray(dv))
    return dv


_SKY_WRT = ("fluxes", "topo", "radec")


def _sky_adjoint(run: _Run, vis, fluxes, full_stokes, single, names, basis: bool):
    """The joint pass of ``simulate_vis_sky_adjoint`` / ``simulate_vis_basis_sky_adjoint``: one device call per time block
    for the flux gradient and the direction gradient together."""
    run = _own_radec_chain(run, "wrt='radec'", "radec" in names, "ask for wrt='topo' and apply its Jacobian",
                           "ask for wrt='topo'")
    f_shape = (run.nsrc, run.nfreqs)
    g, (gflux, gtopo), on_device = _gradient_buffers(run, vis, [
        (f_shape + (2, 2), "complex") if full_stokes else (f_shape, "real"), ((run.ntimes, run.nsrc, 3), "float64")])
    gc, gtopo = _engine_simulate(run, fluxes, force_use_type3=None if basis else True, sky_of=(g, gflux, gtopo))
    res = {"fluxes": stokes_adjoint(gc, full_stokes), "topo": gtopo}
    if "radec" in names:
        res["radec"] = topo_to_radec_gradient(gtopo, _radec_jacobian_of(run))
    return _select({k: v for k, v in res.items() if k in names}, single, names, vis, on_device)


def _sky_full_stokes(run: _Run, fluxes, full_stokes):
    """The forward's fluxes on the host and what their shape says about ``full_stokes`` (a mismatch: ValueError)."""
    fluxes = _host_fluxes(run, fluxes)
    if full_stokes is None:
        full_stokes = fluxes.ndim == 3
    if bool(full_stokes) != (fluxes.ndim == 3):
        raise ValueError(f"full_stokes={full_stokes} does not match fluxes of shape {fluxes.shape}")
    return fluxes, bool(full_stokes)


def simulate_vis_sky_adjoint(
    vis,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    wrt=("fluxes", "radec"),
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    beam_coefs: np.ndarray = None,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Gradients of ``simulate_vis(ants, fluxes, ra, dec, ...)`` with respect to the fluxes AND the source positions from
    one pass, for a visibility-shaped ``vis`` (G = dL/dV, dL = Re sum conj(G) dV) -- what a fit with each source's flux and
    position unknown together needs per step.

    * ``"fluxes"``: ``A^T vis`` as ``simulate_vis_adjoint`` defines it; the fluxes' shape, (nsrc, nfreqs) or
      (nsrc, nfreqs, 4), real, of the run's precision;
    * ``"topo"``: (ntimes, nsrc, 3) float64, ENU, tangential, as ``simulate_vis_source_adjoint`` defines it;
    * ``"radec"``: (nsrc, 2) float64, columns (ra, dec), per radian, under that function's rules: for
      ``coord_method="SiderealRotation"`` and device astrometry; with a ``coord_mgr`` (or a matvis manager the engine would
      build) ValueError: ask for ``"topo"``.

    ``wrt`` is a name or a tuple of distinct names; the result is that gradient, or a tuple in ``wrt``'s order.  With
    ``"fluxes"`` and a position name one joint device call runs per time block (``fv_sim_run_sky_adjoint``): the source
    pass's first transform per (time, frequency group, beam pair) is the flux adjoint's, so its 1 + D transforms serve
    both, where the two separate calls run 2 + D and set up twice.  The flux part is the flux adjoint's own arithmetic on
    those values (it agrees with ``simulate_vis_adjoint`` to rounding in the order of the per-lane sums) and the position
    part is the source pass's, bit for bit.  A ``wrt`` without ``"fluxes"``, or with it alone, runs the single-purpose pass
    and returns its bits.  ``full_stokes`` defaults to what ``fluxes``' shape says.  ``vis`` is a numpy array or a torch
    tensor on the run's device (handed over by pointer; the results are then tensors on that device); host tensors in,
    host tensors out.  Every other keyword means what it means for ``simulate_vis``; ``force_use_type3`` is accepted and
    always on in the joint pass, which runs the type-3 transform (there is no ``adjoint_path``).  Not covered:
    ``beam_coefs`` (NotImplementedError: ``simulate_vis_basis_sky_adjoint``), the antenna positions, multi-GPU."""
    args = locals()
    single, names = _parse_wrt(wrt, _SKY_WRT, "some of 'fluxes', 'topo' and 'radec'")
    if beam_coefs is not None:
        raise NotImplementedError("simulate_vis_sky_adjoint does not support basis beams (beam_coefs): "
                                  "simulate_vis_basis_sky_adjoint does")
    run = _describe_run(args)
    fluxes, full_stokes = _sky_full_stokes(run, fluxes, full_stokes)
    own = {k: v for k, v in args.items() if k not in ("vis", "wrt", "full_stokes", "fluxes", "args")}
    if "fluxes" not in names:
        return simulate_vis_source_adjoint(vis, fluxes=fluxes, wrt=wrt, **own)
    if names == ("fluxes",):
        gf = simulate_vis_adjoint(vis, full_stokes=full_stokes, **own)
        return gf if single else (gf,)
    return _sky_adjoint(run, vis, fluxes, full_stokes, single, names, basis=False)


def simulate_vis_basis_sky_adjoint(
    vis,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    beam_coefs,
    telescope_loc,
    *,
    wrt=("fluxes", "radec"),
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = True,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """``simulate_vis_sky_adjoint`` through basis beams: the gradients of ``simulate_vis(..., beam=<K basis beams>,
    beam_coefs=C)`` with respect to the fluxes and the source positions from one pass
    (``fv_sim_run_basis_sky_adjoint``): the 1 + D transforms per (k <= l) term of ``simulate_vis_basis_source_adjoint``
    also give ``simulate_vis_basis_adjoint(wrt="fluxes")``'s gradient, one transform per term fewer than the two calls.

    ``wrt``, ``full_stokes``, ``vis`` and the results as for ``simulate_vis_sky_adjoint``, the gradients with the meaning
    those two functions give them; a ``wrt`` without ``"fluxes"``, or with it alone, runs the single-purpose pass and
    returns its bits.  ``fluxes`` and ``beam_coefs`` are the forward's; ``polarized`` must be True and ``beam_idx`` None,
    as for the forward.  The coefficients' gradient stays ``simulate_vis_basis_adjoint(wrt="beam_coefs")``'s: its
    transforms run the other way.  Not covered: a lattice form, the antenna positions, multi-GPU."""
    args = locals()
    single, names = _parse_wrt(wrt, _SKY_WRT, "some of 'fluxes', 'topo' and 'radec'")
    if beam_coefs is None:
        raise ValueError("simulate_vis_basis_sky_adjoint needs beam_coefs (without basis beams simulate_vis_sky_adjoint is "
                         "the pass)")
    if not polarized:  # the forward's message
        raise ValueError(
            "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
        )
    run = _describe_run(args)
    fluxes, full_stokes = _sky_full_stokes(run, fluxes, full_stokes)
    own = {k: v for k, v in args.items() if k not in ("vis", "wrt", "full_stokes", "fluxes", "args")}
    if "fluxes" not in names:
        return simulate_vis_basis_source_adjoint(vis, fluxes=fluxes, wrt=wrt, **own)
    if names == ("fluxes",):
        return simulate_vis_basis_adjoint(vis, fluxes=fluxes, wrt=wrt, full_stokes=full_stokes, **own)
    return _sky_adjoint(run, vis, fluxes, full_stokes, single, names, basis=True)


def _basis_sky_autograd_function():
    import torch

    class _SimulateVisBasisSky(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, beam_coefs, radec, kwargs):
            ctx.kwargs = kwargs
            ctx.flux_dtype, ctx.coef_dtype, ctx.pos_dtype = fluxes.dtype, beam_coefs.dtype, radec.dtype
            ctx.coef_device, ctx.pos_device = beam_coefs.device, radec.device
            ctx.save_for_backward(fluxes, beam_coefs, radec)
            ctx.save_for_forward(fluxes, beam_coefs, radec)
            return _forward_tensor(dict(kwargs, **_radec_columns(radec)), fluxes=fluxes, beam_coefs=beam_coefs)

        @staticmethod
        def backward(ctx, grad_output):
            fluxes, beam_coefs, radec = ctx.saved_tensors
            pos = _radec_columns(radec)
            wrt = tuple(n for n, need in zip(("fluxes", "beam_coefs"), ctx.needs_input_grad[:2]) if need)
            got, gp = {}, None
            if ctx.needs_input_grad[0] and ctx.needs_input_grad[2]:  # one pass for the fluxes and the positions
                got["fluxes"], gp = simulate_vis_basis_sky_adjoint(grad_output, fluxes=fluxes, beam_coefs=beam_coefs,
                                                                   wrt=("fluxes", "radec"), **pos, **ctx.kwargs)
                if ctx.needs_input_grad[1]:
                    got["beam_coefs"], = simulate_vis_basis_adjoint(grad_output, fluxes=fluxes, beam_coefs=beam_coefs,
                                                                    wrt=("beam_coefs",), **pos, **ctx.kwargs)
                wrt = ()
            if wrt:
                got = dict(zip(wrt, simulate_vis_basis_adjoint(grad_output, fluxes=fluxes, beam_coefs=beam_coefs, wrt=wrt,
                                                               **pos, **ctx.kwargs)))
            if ctx.needs_input_grad[2] and gp is None:
                gp = simulate_vis_basis_source_adjoint(grad_output, fluxes=fluxes, beam_coefs=beam_coefs, wrt="radec",
                                                       **pos, **ctx.kwargs)
            return (_as_grad(got.get("fluxes"), grad_output.device, ctx.flux_dtype),
                    _as_grad(got.get("beam_coefs"), ctx.coef_device, ctx.coef_dtype),
                    _as_grad(gp, ctx.pos_device, ctx.pos_dtype), None)

        @staticmethod
        def jvp(ctx, d_fluxes, d_beam_coefs, d_radec, _):
            fluxes, beam_coefs, radec = ctx.saved_tensors
            pos = _radec_columns(radec)
            if d_fluxes is None and d_beam_coefs is None and d_radec is None:
                return None
            dv = None
            if d_fluxes is not None or d_beam_coefs is not None:
                dv = _tangent_tensor(simulate_vis_basis_jvp(fluxes=fluxes, beam_coefs=beam_coefs, **pos,
                                                            **_detached(d_beam_coefs=d_beam_coefs, d_fluxes=d_fluxes),
                                                            **ctx.kwargs), fluxes)
            if d_radec is not None:
                ds = _tangent_tensor(simulate_vis_basis_source_jvp(fluxes=fluxes, beam_coefs=beam_coefs, **pos,
                                                                   **_detached(d_radec=d_radec), **ctx.kwargs), fluxes)
                dv = ds if dv is None else dv + ds
            return dv

    return _SimulateVisBasisSky


def torch_simulate_vis_basis_sky(fluxes, beam_coefs, radec, **kwargs):
    """The basis-beam simulation as a torch operation differentiable in the fluxes, the coefficients and the source
    positions -- the unknowns of a joint beam and catalogue fit: ``fluxes`` real, (nsrc, nfreqs) or (nsrc, nfreqs, 4);
    ``beam_coefs`` complex, (nant, nbasis, nfreqs); ``radec`` real, (nsrc, 2), columns (ra, dec) in radians.  Every other
    argument is a keyword of ``simulate_vis`` -- but for ``ra`` and ``dec``, which the tensor replaces (TypeError).  Returns
    the visibilities as a complex tensor on ``fluxes``' device.  The backward pass runs only what autograd asks for
    (``ctx.needs_input_grad``): one ``simulate_vis_basis_adjoint`` call for the fluxes and / or the coefficients,
    ``simulate_vis_basis_source_adjoint(wrt="radec")`` for the positions, which needs ``coord_method="SiderealRotation"`` or
    device astrometry; when the fluxes and the positions are both asked for, one ``simulate_vis_basis_sky_adjoint`` call
    serves the two (and ``simulate_vis_basis_adjoint(wrt=("beam_coefs",))`` the coefficients).  Forward mode (``torch.autograd.forward_ad``) runs ``simulate_vis_basis_jvp`` and
    ``simulate_vis_basis_source_jvp`` on the tangents present, under the same condition."""
    if "ra" in kwargs or "dec" in kwargs:
        raise TypeError("torch_simulate_vis_basis_sky takes the source positions as the tensor radec, not ra= / dec=")
    if radec.ndim != 2 or radec.shape[1] != 2 or radec.is_complex():
        raise ValueError(f"radec must be a real (nsrc, 2) tensor, got {tuple(radec.shape)} {radec.dtype}")
    return _function(_basis_sky_autograd_function).apply(fluxes, beam_coefs, radec, kwargs)


_CHI2_WRT = ("fluxes", "ants", "baselines", "topo", "radec", "beam_coefs", "gains")


def _gain_block(run: _Run, gains) -> np.ndarray:
    """``simulate_vis_gain_chi2``'s ``gains`` -- (nant, [2,] nfreqs[, ntimes]) complex, rows in ``ants``' order -- checked and
    broadcast to the block layout the engine takes: (nfreqs, ntimes, nfeed, nant), C-contiguous, the run's complex dtype."""
    g = _host(gains)
    nant, nfeed = len(run.ants), 2 if run.args["polarized"] else 1
    lead = (nant, 2) if nfeed == 2 else (nant,)
    shapes = (lead + (run.nfreqs,), lead + (run.nfreqs, run.ntimes))
    if not np.iscomplexobj(g):
        raise ValueError("gains must be complex (one gain per antenna, feed and channel)")
    if g.shape not in shapes:
        raise ValueError(f"gains must have shape {shapes[0]} or {shapes[1]}, got {g.shape}")
    if not np.isfinite(g).all():
        raise ValueError("gains must be finite")
    g = g.reshape(nant, nfeed, run.nfreqs, -1)
    g = np.broadcast_to(g, (nant, nfeed, run.nfreqs, run.ntimes))
    return np.ascontiguousarray(g.transpose(2, 3, 1, 0), dtype=run.cdt)


def _gain_gradient(run: _Run, ggains: np.ndarray, shape) -> np.ndarray:
    """The engine's (nfreqs, ntimes, nfeed, nant) gain gradient in the shape the gains were given in; for time-constant
    gains the per-time gradients are added in time order."""
    g = ggains.transpose(3, 2, 0, 1)  # (nant, nfeed, nfreqs, ntimes)
    if len(shape) == g.ndim - (0 if run.args["polarized"] else 1):  # per-time gains
        return np.ascontiguousarray(g).reshape(shape)
    total = np.zeros(g.shape[:-1], dtype=np.complex128)
    for t in range(g.shape[-1]):
        total += g[..., t]
    return total.reshape(shape)


def _jones_block(run: _Run, jones) -> np.ndarray:
    """``simulate_vis_jones_chi2``'s ``jones`` -- (nant, 2, 2, nfreqs[, ntimes]) complex, rows in ``ants``' order -- checked
    and broadcast to the block layout the engine takes: (nfreqs, ntimes, 2, 2, nant), C-contiguous, the run's complex dtype."""
    j = _host(jones)
    nant = len(run.ants)
    shapes = ((nant, 2, 2, run.nfreqs), (nant, 2, 2, run.nfreqs, run.ntimes))
    if not np.iscomplexobj(j):
        raise ValueError("jones must be complex (one 2 x 2 matrix per antenna and channel)")
    if j.shape not in shapes:
        raise ValueError(f"jones must have shape {shapes[0]} or {shapes[1]}, got {j.shape}")
    if not np.isfinite(j).all():
        raise ValueError("jones must be finite")
    j = np.broadcast_to(j.reshape(nant, 2, 2, run.nfreqs, -1), (nant, 2, 2, run.nfreqs, run.ntimes))
    return np.ascontiguousarray(j.transpose(3, 4, 1, 2, 0), dtype=run.cdt)


def _jones_gradient(run: _Run, gjones: np.ndarray, shape) -> np.ndarray:
    """The engine's (nfreqs, ntimes, 2, 2, nant) gradient in the shape the matrices were given in; for time-constant
    matrices the per-time gradients are added in time order."""
    g = gjones.transpose(4, 2, 3, 0, 1)  # (nant, 2, 2, nfreqs, ntimes)
    if len(shape) == g.ndim:  # per-time matrices
        return np.ascontiguousarray(g)
    total = np.zeros(g.shape[:-1], dtype=np.complex128)
    for t in range(g.shape[-1]):
        total += g[..., t]
    return total


# ---- what the fit entry points share: simulate_vis_gain_chi2, simulate_vis_gain_gauss_newton, simulate_vis_gain_solve ----

def _fit_keywords(wrt, gains, per_name, per, adjoint_path, beam_coefs, polarized, d_beam_coefs=None, kind="gains"):
    """The keywords ``simulate_vis_gain_chi2``, ``simulate_vis_jones_chi2`` and ``simulate_vis_gain_gauss_newton`` check
    alike, before the run is described; ``per_name`` names the caller's ``chi2_per`` / ``quad_per``, ``kind`` the keyword
    ``gains`` came by and the name ``wrt`` has for it.  Returns ``wrt`` as (single, names)."""
    single = isinstance(wrt, str)
    names = (wrt,) if single else tuple(wrt)
    if names:
        _parse_wrt(wrt, _CHI2_WRT[:-1] + (kind,),
                   f"some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and '{kind}'")
    if kind in names and gains is None:
        raise ValueError(f"wrt='{kind}' needs {kind}=")
    if per not in ("total", "freq_time"):
        raise ValueError(f"{per_name} must be 'total' or 'freq_time', got {per!r}")
    if adjoint_path not in ("type3", "type2", "auto"):
        raise ValueError(f"adjoint_path must be 'type3', 'type2' or 'auto', got {adjoint_path!r}")
    if d_beam_coefs is not None and beam_coefs is None:
        raise ValueError("d_beam_coefs needs beam_coefs (basis beams)")
    if "beam_coefs" in names and beam_coefs is None:
        raise ValueError("wrt='beam_coefs' needs beam_coefs (basis beams)")
    if beam_coefs is not None and not polarized:  # the forward's message
        raise ValueError(
            "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
        )
    return single, names


def _check_vis_block(run: _Run, x, name):
    """``data`` or ``model``: on the host or on the run's device, in ``simulate_vis``'s output shape."""
    _run_device(run, (x,), name)
    if tuple(x.shape) != run.vis_shape:
        raise ValueError(f"{name} must have simulate_vis's output shape {run.vis_shape}, got {tuple(x.shape)}")


def _check_weights(run: _Run, weights, whose):
    """``weights`` (not None): real, in the shape the caller's message calls ``whose`` shape."""
    if tuple(weights.shape) != run.vis_shape:
        raise ValueError(f"weights must have {whose} shape {run.vis_shape}, got {tuple(weights.shape)}")
    if weights.is_complex() if _is_tensor(weights) else np.iscomplexobj(weights):
        raise ValueError("weights must be real (inverse variances; 0 flags a sample)")


def _fit_outputs(run: _Run, names, full_stokes):
    """``_gradient_buffers``' specification of the fit passes' four gradient buffers -- gflux, gcoefs, gbls, gtopo --, None
    for one no name of ``wrt`` needs."""
    f_shape = (run.nsrc, run.nfreqs)
    return [
        None if "fluxes" not in names else (f_shape + (2, 2), "complex") if full_stokes else (f_shape, "real"),
        None if "beam_coefs" not in names else (run.beam_coefs.shape, "complex"),
        None if "ants" not in names and "baselines" not in names else ((run.nbls, 3), "float64"),
        None if "topo" not in names and "radec" not in names else ((run.ntimes, run.nsrc, 3), "float64")]


def _gvis_buffer(run: _Run, return_gvis):
    """The zeroed device tensor G is returned in, complete before the library writes it; None when it is not asked for."""
    if not return_gvis:
        return None
    import torch

    gvis = _zeros(torch.device("cuda", int(run.args["device"])), run.vis_shape, run.cdt)
    _synchronize(gvis.device)
    return gvis


def _fit_gradients(run: _Run, single, names, buffers, full_stokes, ggains, gains, like, device, kind="gains"):
    """What a fit call returns for ``wrt`` out of the engine's ``buffers`` (gflux, gcoefs, gbls, gtopo) and its gain block
    ``ggains``: the gains' gradient in ``gains``' own shape (``kind="jones"``: the matrices'), Stokes fluxes, the radec
    chain, the antenna fold.  The outputs follow ``like`` (the tensor among the inputs, or None) and live on the torch
    ``device`` (None: the host)."""
    gflux, gcoefs, gbls, gtopo = buffers
    res = {"topo": gtopo, "baselines": gbls, "beam_coefs": gcoefs}
    if kind in names:
        res[kind] = (_jones_gradient if kind == "jones" else _gain_gradient)(run, ggains, tuple(gains.shape))
        if device is not None:
            import torch

            res[kind] = torch.from_numpy(res[kind]).to(device)
    if "fluxes" in names:
        res["fluxes"] = stokes_adjoint(gflux, full_stokes)
    if "radec" in names:
        res["radec"] = topo_to_radec_gradient(gtopo, _radec_jacobian_of(run))
    if "ants" in names:
        res["ants"] = baseline_to_antenna_gradient(gbls, run.ants, run.baselines)
    return _select({k: v for k, v in res.items() if k in names}, single, names, like, device is not None) if names else ()


def _fit_value(rows: np.ndarray, per, like, device):
    """The engine's (nfreqs, ntimes) float64 ``rows`` as the caller's ``chi2_per`` / ``quad_per`` asks: "total" their sum as
    a Python float, added in row-major order, else the array itself, following ``like`` and ``device`` as the gradients
    do."""
    if per == "total":
        return float(np.cumsum(rows.ravel())[-1])
    if like is None:
        return rows
    import torch

    value = torch.from_numpy(rows)
    return value if device is None else value.to(device)


def _gvis_home(gvis, like, device):
    """G as it is returned: the device tensor for a run on the device, else on the host, a tensor when ``like`` is one."""
    if device is not None:
        return gvis
    gvis = gvis.cpu().numpy()
    if like is not None:
        import torch

        gvis = torch.from_numpy(gvis)
    return gvis


def simulate_vis_chi2(
    data,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    weights=None,
    wrt=("fluxes",),
    beam_coefs=None,
    chi2_per: str = "total",
    return_gvis: bool = False,
    adjoint_path: str = "type3",
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """The fit objective and its gradients in one call: ``chi2 = sum w |V - data|^2`` with ``V = simulate_vis(ants, fluxes,
    ra, dec, ...)`` of the same arguments, and the gradients of chi2 (not of chi2 / 2) with respect to the parameters
    named in ``wrt``.  One handle and one set-up serve the forward run and every derivative pass, and the visibilities
    never leave the device: per time block the forward writes them into a device buffer, a residual kernel replaces them
    by ``G = 2 w (V - data) = d chi2 / dV`` and adds up chi2 (``fv_sim_run_residual``), and the handle passes of the
    public adjoints read G where it lies.  Returns ``(chi2, grads)``, with ``return_gvis=True`` ``(chi2, grads, G)``.

    * ``data``: ``simulate_vis``'s output shape.  ``weights``: None (every weight 1) or a real array of that shape, inverse
      variances; a weight of exactly 0 flags its sample: it adds nothing, G is exactly 0 there and the datum is not used
      (it may be NaN).  A negative or non-finite weight, or a non-finite datum at a positive weight, fails the call.  Both
      may be numpy arrays or torch tensors; tensors on the run's device are read by pointer and may stay resident across
      the iterations of a fit (ValueError for another device).  The outputs follow ``data`` as the outputs of the other
      passes follow ``vis``: tensors on its device for a device tensor, host tensors for a host tensor, numpy otherwise.
    * ``wrt``: a name or a tuple of distinct names out of ``"fluxes"``, ``"ants"``, ``"baselines"``, ``"topo"``, ``"radec"``
      and, with ``beam_coefs`` (basis beams; ``polarized=True``), ``"beam_coefs"``; ``grads`` is that gradient, or a tuple in
      ``wrt``'s order.  Shapes, units and the coordinate rules of ``"radec"`` are those of the public pass that owns the
      name (``simulate_vis_sky_adjoint``, ``simulate_vis_position_adjoint``, ``simulate_vis_basis_adjoint``,
      ``simulate_vis_basis_sky_adjoint``), whose handle pass runs here on G, so the gradients are those functions' results
      for ``vis = G``.  ``wrt=()`` gives the value alone (a line search) and ``grads == ()``.
    * ``chi2_per="total"``: a Python float, the sum of the (nfreqs, ntimes) array in row-major order; ``"freq_time"``: that
      float64 array, one value per (frequency, time) -- bitwise reproducible for a given forward result (no
      floating-point atomics).
    * ``return_gvis=True`` appends G in ``data``'s shape, what a Gauss-Newton step needs: ``J^T W r = J^T G / 2``.
    * ``adjoint_path``: as for ``simulate_vis_adjoint``, for ``wrt`` within ``{"fluxes"}``.
    * ``force_use_type3`` is honoured for ``wrt`` within ``{"fluxes"}`` -- a lattice array then takes the type-1 forward --
      and is ON FOR THE WHOLE CALL otherwise: the position passes run the type-3 transform and share the handle with the
      forward, so the forward of such a call is the type-3 one (equal to the type-1 result to ``eps``).

    Every other keyword means what it means for ``simulate_vis``.  Uncalibrated data -- per-antenna complex gains in the data
    model, and the gradient with respect to them -- are ``simulate_vis_gain_chi2``'s, this call with ``gains=``.  Not
    covered: forward-mode derivatives, a tangent in the same call (``simulate_vis_gauss_newton`` is the J^T W J product),
    sharding over GPUs."""
    own = locals()
    if isinstance(wrt, str) or tuple(wrt):  # (its own names: "gains" is simulate_vis_gain_chi2's)
        _parse_wrt(wrt, _CHI2_WRT[:-1], "some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs'")
    return simulate_vis_gain_chi2(gains=None, **own)


def simulate_vis_gain_chi2(
    data,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    gains,
    weights=None,
    wrt=("fluxes",),
    beam_coefs=None,
    chi2_per: str = "total",
    return_gvis: bool = False,
    adjoint_path: str = "type3",
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """``simulate_vis_chi2`` for uncalibrated data: one complex gain per antenna, feed, channel and optionally time in the
    data model.  Baseline (a1, a2) is modelled as ``V' = conj(g[a1]) g[a2] V`` -- the first antenna is the conjugated one, as
    for ``beam_coefs`` --, ``chi2 = sum w |V' - data|^2``, and ``"gains"`` is one more name ``wrt`` takes.  The product is
    applied on the device to the block the residual kernel touches (``fv_sim_run_residual_gains``), whatever path produced
    V; everything else -- ``data``, ``weights``, the other names of ``wrt``, ``chi2_per``, ``adjoint_path``,
    ``force_use_type3``, the returned tuple -- is ``simulate_vis_chi2``'s, which is this call with ``gains=None``.

    * ``gains``: ``(nant, nfreqs)`` or per time ``(nant, nfreqs, ntimes)``; polarized ``(nant, 2, nfreqs)`` or
      ``(nant, 2, nfreqs, ntimes)``, one gain per feed: the polarized output ``[f, t, x, y, k]`` is multiplied by
      ``conj(g[a1, y]) g[a2, x]``, which is what replacing each antenna's Jones matrix ``A_a[ax, feed]`` by
      ``A_a diag(g[a])`` does.  Rows follow ``ants``' iteration order.  Complex, finite; numpy or a tensor on any device (it
      is small and goes through the host).
    * ``"gains"`` in ``wrt`` gives the gradient in ``gains``' own shape, complex128, in torch's convention for a complex leaf,
      ``d chi2 = Re sum conj(grad) d gains`` (the convention of the ``beam_coefs`` gradient), following ``data`` as the
      other gradients do; for time-constant gains it is the per-time gradients added on the host in time order.  Every
      other gradient is its public pass's result for ``vis = G``.
    * ``return_gvis=True`` gives that ``G = d chi2 / dV = conj(m) 2 w (V' - data)``, ``m`` the gain product -- NOT
      ``2 w (V' - data)``.
    * With the default ``baselines=None`` there is one baseline per redundant group and the gains applied are those of each
      group's representative pair: a calibration passes explicit ``baselines``.

    The Gauss-Newton product of this chi2 is ``simulate_vis_gain_gauss_newton``'s (``simulate_vis_gauss_newton`` itself
    takes no gains), and the gains that minimise it for a fixed model are ``simulate_vis_gain_solve``'s.  Not covered:
    gains in ``simulate_vis`` itself, ``model=`` in this call, sharding over GPUs.  Full 2x2 Jones (leakage) matrices per
    antenna are ``simulate_vis_jones_chi2``'s."""
    return _gain_chi2(locals(), "gains")


def _gain_chi2(args: dict, kind: str):
    """``simulate_vis_gain_chi2`` (``kind="gains"``) and ``simulate_vis_jones_chi2`` (``kind="jones"``): ``args`` is the
    public function's ``locals()``, ``args[kind]`` its gains or matrices (None: neither, ``simulate_vis_chi2``).  The two
    differ in the block the engine's objective pass is given, in the output that receives its gradient and in the name
    ``wrt`` has for it."""
    gains, data, weights, return_gvis = args[kind], args["data"], args["weights"], args["return_gvis"]
    single, names = _fit_keywords(args["wrt"], gains, "chi2_per", args["chi2_per"], args["adjoint_path"], args["beam_coefs"],
                                  args["polarized"], kind=kind)
    if kind == "jones" and not args["polarized"]:
        raise ValueError("jones needs polarized=True: a 2 x 2 matrix per antenna mixes the two feeds")
    run = _describe_run(args)
    run = _own_radec_chain(run, "wrt='radec'", "radec" in names, "ask for wrt='topo' and apply its Jacobian",
                           "ask for wrt='topo'")
    fluxes, full_stokes = _sky_full_stokes(run, args["fluxes"], args["full_stokes"])
    _check_vis_block(run, data, "data")
    if weights is not None:
        _check_weights(run, weights, "data's")
    gain_block = None if gains is None else (_jones_block if kind == "jones" else _gain_block)(run, gains)
    ggains = np.zeros(gain_block.shape, dtype=np.complex128) if kind in names else None
    d, buffers, on_device = _gradient_buffers(run, data, _fit_outputs(run, names, full_stokes))
    w = None
    if weights is not None:
        w_device = _run_device(run, (weights,), "weights")
        w = _host(weights).astype(run.rdt, copy=False) if w_device is None else _on(w_device, weights, run.rdt)
        _synchronize(w_device)
    gvis = _gvis_buffer(run, return_gvis)
    outputs = dict(zip(("gflux", "gcoefs", "gbls", "gtopo"), buffers), gvis=gvis)
    if gains is None:
        objective_of = (d, w, outputs)
    elif kind == "jones":
        objective_of = (d, w, dict(outputs, gjones=ggains), ("jones", gain_block))
    else:
        objective_of = (d, w, dict(outputs, ggains=ggains), gain_block)
    chi2_ft = _engine_simulate(
        run, fluxes, force_use_type3=None if set(names) <= {"fluxes"} else True, adjoint_path=args["adjoint_path"],
        objective_of=objective_of)
    like, dev = data if _is_tensor(data) else None, data.device if on_device else None
    grads = _fit_gradients(run, single, names, buffers, full_stokes, ggains, gains, like, dev, kind=kind)
    chi2 = _fit_value(chi2_ft, args["chi2_per"], like, dev)
    return (chi2, grads, _gvis_home(gvis, like, dev)) if return_gvis else (chi2, grads)


def simulate_vis_jones_chi2(
    data,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    jones,
    weights=None,
    wrt=("fluxes",),
    beam_coefs=None,
    chi2_per: str = "total",
    return_gvis: bool = False,
    adjoint_path: str = "type3",
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """``simulate_vis_chi2`` with one 2 x 2 complex matrix per antenna, channel and optionally time in the data model: the
    gains of the two feeds on its diagonal and the leakage of each feed into the other (D-terms) off it.  Antenna ``a``'s
    Jones matrix ``A_a[ax, feed]`` becomes ``A_a jones[a]``, so that on the polarized output ``[f, t, x, y, k]`` of baseline
    ``k = (a1, a2)``

        ``V'[x, y] = sum_{x', y'} conj(jones[a1][y', y]) jones[a2][x', x] V[x', y']``,

    ``chi2 = sum w |V' - data|^2``, and ``"jones"`` is one more name ``wrt`` takes.  The product is applied on the device to
    the block the residual kernel touches (``fv_sim_run_residual_jones``), whatever path produced V; everything else --
    ``data``, ``weights``, the other names of ``wrt``, ``chi2_per``, ``adjoint_path``, ``force_use_type3``, the returned
    tuple -- is ``simulate_vis_chi2``'s.  ``jones[a] = diag(gains[a])`` is ``simulate_vis_gain_chi2``.

    * Needs ``polarized=True`` (ValueError otherwise).
    * ``jones``: ``(nant, 2, 2, nfreqs)`` or per time ``(nant, 2, 2, nfreqs, ntimes)``; ``jones[a, i, j]`` has ``i`` the feed
      of the ideal antenna and ``j`` the measured feed.  Rows follow ``ants``' iteration order.  Complex, finite; numpy or a
      tensor on any device (it is small and goes through the host).
    * ``"jones"`` in ``wrt`` gives the gradient in ``jones``' own shape, complex128, in torch's convention for a complex
      leaf, ``d chi2 = Re sum conj(grad) d jones`` (the convention of the ``gains`` and ``beam_coefs`` gradients), following
      ``data`` as the other gradients do; for time-constant matrices it is the per-time gradients added on the host in time
      order.  Every other gradient is its public pass's result for ``vis = G``.
    * ``return_gvis=True`` gives that ``G = d chi2 / dV``, the transposed product applied to ``2 w (V' - data)`` -- NOT
      ``2 w (V' - data)`` itself.
    * A weight of 0 flags that one ``(x, y)`` sample; the baseline's other samples still use all four model values.
    * With the default ``baselines=None`` there is one baseline per redundant group and the matrices applied are those of
      each group's representative pair: a calibration passes explicit ``baselines``.
    * The device holds one more fp64 value per visibility of a time block (the rows' terms of chi2), which the time
      blocks are sized for.

    The Gauss-Newton product of this chi2 is ``simulate_vis_jones_gauss_newton``'s, and the matrices that minimise it for a
    fixed model are ``simulate_vis_jones_solve``'s.  Not covered: ``model=`` in this call, sharding over GPUs."""
    return _gain_chi2(locals(), "jones")


def _chi2_autograd_function():
    import torch
    from torch.autograd.function import once_differentiable

    class _SimulateVisChi2(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, beam_coefs, antpos, radec, gains, data, weights, antnums, kwargs, kind):
            inputs = (("fluxes", fluxes), ("beam_coefs", beam_coefs), ("ants", antpos), ("radec", radec), (kind, gains))
            wrt = tuple(n for (n, _), need in zip(inputs, ctx.needs_input_grad[:5]) if need)
            kw = dict(kwargs)
            call = simulate_vis_chi2
            if gains is not None:
                call, kw[kind] = (simulate_vis_jones_chi2 if kind == "jones" else simulate_vis_gain_chi2), gains
            if antpos is not None:
                kw["ants"] = _ants_of(antnums, antpos)
            if radec is not None:
                kw.update(_radec_columns(radec))
            chi2, grads = call(data, fluxes=fluxes, weights=weights, beam_coefs=beam_coefs, wrt=wrt, chi2_per="total", **kw)
            got = dict(zip(wrt, grads))
            ctx.grads = tuple(None if got.get(n) is None else _as_grad(got[n], x.device, x.dtype) for n, x in inputs)
            return torch.tensor(chi2, dtype=torch.float64, device=fluxes.device)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            return tuple(None if g is None else g * grad_output.to(device=g.device, dtype=g.real.dtype)
                         for g in ctx.grads) + (None,) * 5

    return _SimulateVisChi2


def torch_simulate_vis_chi2(data, fluxes, *, weights=None, beam_coefs=None, antpos=None, antnums=None, radec=None, **kwargs):
    """``simulate_vis_chi2`` as a torch loss: ``chi2 = sum w |V - data|^2`` as a scalar float64 tensor on ``fluxes``' device,
    differentiable in ``fluxes`` (real, (nsrc, nfreqs) or (nsrc, nfreqs, 4)) and in the optional tensors ``beam_coefs``
    (complex, (nant, nbasis, nfreqs): basis beams), ``antpos`` (real, (nant, 3), ENU metres, replacing ``ants=``; ``antnums``
    gives the keys ``baselines`` refers to) and ``radec`` (real, (nsrc, 2), replacing ``ra=`` / ``dec=``; needs
    ``coord_method="SiderealRotation"`` or device astrometry).  ``data`` and ``weights`` are constants, numpy arrays or
    tensors -- tensors on the run's device stay there; every other argument is a keyword of ``simulate_vis_chi2``.  The
    forward reads ``ctx.needs_input_grad`` and makes ONE ``simulate_vis_chi2`` call with exactly the inputs that need a
    gradient, keeping the gradients; the backward pass multiplies them by the incoming scalar (once differentiable).
    ``gains=`` (``simulate_vis_gain_chi2``'s per-antenna gains, whose call the forward then makes) may be a complex tensor on any device: one that requires a
    gradient adds ``"gains"`` to that one call and receives its ``.grad`` in its own dtype and on its own device; a
    constant tensor or an array is passed through.  ``jones=`` (``simulate_vis_jones_chi2``'s 2 x 2 matrices per antenna)
    is taken the same way, with ``"jones"`` in place of ``"gains"``; ``gains=`` and ``jones=`` together are a TypeError.  Not
    covered: forward-mode differentiation, double backward."""
    for taken, by in (("wrt", "what requires a gradient"), ("chi2_per", "the scalar loss"), ("return_gvis", "the scalar loss")):
        if taken in kwargs:
            raise TypeError(f"torch_simulate_vis_chi2 does not take {taken}=: {by} decides")
    if antpos is not None:
        antnums = _checked_antnums("torch_simulate_vis_chi2", antpos, antnums, kwargs)
    elif antnums is not None:
        raise TypeError("antnums goes with the tensor antpos")
    if radec is not None:
        if "ra" in kwargs or "dec" in kwargs:
            raise TypeError("torch_simulate_vis_chi2 takes the source positions as the tensor radec or as ra= / dec=, not both")
        if radec.ndim != 2 or radec.shape[1] != 2 or radec.is_complex():
            raise ValueError(f"radec must be a real (nsrc, 2) tensor, got {tuple(radec.shape)} {radec.dtype}")
    kwargs = dict(kwargs)
    gains, jones = kwargs.pop("gains", None), kwargs.pop("jones", None)
    if gains is not None and jones is not None:
        raise TypeError("torch_simulate_vis_chi2 takes gains= or jones=, not both (diagonal matrices are the gains)")
    kind = "gains" if jones is None else "jones"
    return _function(_chi2_autograd_function).apply(fluxes, beam_coefs, antpos, radec, gains if jones is None else jones,
                                                    data, weights, antnums, kwargs, kind)


_GAUSS_NEWTON_NAMES = (("d_ants", "ants"), ("d_baselines", "baselines"), ("d_radec", "radec"), ("d_topo", "topo"),
                       ("d_fluxes", "fluxes"), ("d_beam_coefs", "beam_coefs"))


def simulate_vis_gauss_newton(
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    d_fluxes=None,
    d_ants=None,
    d_baselines=None,
    d_radec=None,
    d_topo=None,
    d_beam_coefs=None,
    weights=None,
    wrt=None,
    quad_per: str = "total",
    return_gvis: bool = False,
    adjoint_path: str = "type3",
    beam_coefs=None,
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """The Gauss-Newton product in one call: with J the Jacobian of ``V = simulate_vis(ants, fluxes, ra, dec, ...)`` and
    ``U = J p`` the tangent along the direction ``p`` given by the ``d_*`` arguments -- the sum of the tangents exactly as
    ``simulate_vis_jvp``, ``simulate_vis_basis_jvp`` and ``simulate_vis_basis_source_jvp`` define them -- returns
    ``(quad, prods)``, with ``return_gvis=True`` ``(quad, prods, G)``:

    * ``quad = sum w |U|^2``: a Python float, or with ``quad_per="freq_time"`` the (nfreqs, ntimes) float64 array, one value
      per (frequency, time), bitwise reproducible for given tangents (no floating-point atomics); the total is the sum of
      that array in row-major order;
    * ``G = 2 w U`` in ``simulate_vis``'s shape;
    * ``prods``: the public adjoints' results for ``vis = G``, for the names in ``wrt`` -- that is ``H p`` restricted to
      those parameter blocks, ``H = 2 J^T W J`` the Gauss-Newton Hessian of ``simulate_vis_chi2``'s chi2: ``x`` solving
      ``H x = -grad`` is the Gauss-Newton step, and ``<p, H p> = 2 quad``.

    One handle and one set-up serve every pass, and U never leaves the device: per time block every tangent pass fills a
    device block -- the forward on ``d_fluxes``, ``fv_sim_run_basis_tangent``, ``fv_sim_run_tangent`` or
    ``fv_sim_run_basis_position_tangent``, ``fv_sim_run_basis_source_tangent`` --, one kernel sums them in that order,
    weights the sum into G and adds up the rows of ``quad`` (``fv_sim_weight_block``), and the handle passes of the public
    adjoints read G where it lies, as in ``simulate_vis_chi2``.

    * Directions, with the shapes and rules of the jvp functions: ``d_fluxes`` (``fluxes``' shape); ``d_ants`` (nant, 3) or
      ``d_baselines`` (nbls, 3), not both; ``d_radec`` (nsrc, 2) -- ``coord_method="SiderealRotation"`` or device astrometry
      -- or ``d_topo`` (ntimes, nsrc, 3), not both; ``d_beam_coefs``, complex (nant, nbasis, nfreqs), with ``beam_coefs``
      (basis beams; ``polarized=True``) -- one direction: a stack is a ValueError.  No direction at all is a ValueError.
    * ``weights``: None (every weight 1) or a real array of ``simulate_vis``'s output shape, inverse variances; a weight of
      exactly 0 flags its sample (G exactly 0, nothing added, U not used there); a negative or non-finite weight fails
      the call.
    * ``wrt``: ``simulate_vis_chi2``'s names, rules and shapes, ``"radec"``'s coordinate rules included; ``prods`` is that
      product, or a tuple in ``wrt``'s order.  ``wrt=None``: the names whose directions were given (``d_ants`` ->
      ``"ants"``, ``d_baselines`` -> ``"baselines"``, ``d_radec`` -> ``"radec"``, ``d_topo`` -> ``"topo"``, ``d_fluxes`` ->
      ``"fluxes"``, ``d_beam_coefs`` -> ``"beam_coefs"``), in that order, always a tuple.
    * Weights and directions may be numpy arrays or torch tensors; tensors on the run's device are read by pointer
      (``d_fluxes``, ``d_ants`` and ``d_radec`` pass through the host).  The outputs follow them as ``simulate_vis_chi2``'s
      follow ``data``: tensors on the run's device when any of them is one, host tensors for host tensors, numpy otherwise.
    * ``adjoint_path`` and ``force_use_type3`` are honoured when ``d_fluxes`` is the only direction and ``wrt`` is within
      ``{"fluxes"}`` -- a lattice array then takes the type-1 forward --; with any other direction or name the whole call
      runs the type-3 transform.

    Every other keyword means what it means for ``simulate_vis``.  Uncalibrated data -- per-antenna gains in the data
    model, a gain direction and the gain block of ``H p`` -- are ``simulate_vis_gain_gauss_newton``'s, this call with
    ``gains=`` and ``d_gains=``.  Not covered: the gradient in the same call
    (``simulate_vis_chi2``), damping (``H + lambda D`` is an axpy on the host), several directions per call, torch ``hvp``,
    sharding over GPUs."""
    own = locals()
    if wrt is not None and (isinstance(wrt, str) or tuple(wrt)):  # (its own names: "gains" is simulate_vis_gain_gauss_newton's)
        _parse_wrt(wrt, _CHI2_WRT[:-1], "some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs'")
    return simulate_vis_gain_gauss_newton(gains=None, **own)


def simulate_vis_gain_gauss_newton(
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    gains,
    d_fluxes=None,
    d_ants=None,
    d_baselines=None,
    d_radec=None,
    d_topo=None,
    d_beam_coefs=None,
    d_gains=None,
    weights=None,
    wrt=None,
    quad_per: str = "total",
    return_gvis: bool = False,
    adjoint_path: str = "type3",
    beam_coefs=None,
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """``simulate_vis_gauss_newton`` for uncalibrated data: the Gauss-Newton product of ``simulate_vis_gain_chi2``'s chi2,
    whose data model is ``V' = conj(g[a1]) g[a2] V``, along a joint direction ``p = (sky directions, d_gains)``, the gain
    block of ``H p`` included.  With ``m`` the gain product, ``dm = conj(dg[a1]) g[a2] + conj(g[a1]) dg[a2]`` its tangent and
    ``U`` the sky tangent as ``simulate_vis_gauss_newton`` defines it, the tangent of the data model is
    ``U' = m U + dm V``; ``quad = sum w |U'|^2``, ``H = 2 J'^T W J'`` with ``J'`` the Jacobian of V', and
    ``<p, H p> = 2 quad``, the gains' part of the inner product being ``Re sum conj(d_gains) prod``.  The product is applied
    on the device to the blocks the weighting kernel touches (``fv_sim_gain_weight_block``), whatever path produced them;
    everything else -- the ``d_*`` directions, ``weights``, the other names of ``wrt``, ``quad_per``, ``adjoint_path``,
    ``force_use_type3``, the returned tuple -- is ``simulate_vis_gauss_newton``'s, which is this call with ``gains=None``.

    * ``gains``: ``simulate_vis_gain_chi2``'s, with its shapes and rules.  ``d_gains``: the gain direction, ``gains``' own
      shape -- time-constant or per time as ``gains`` is --, complex and finite, or None.  ``d_gains`` alone is a valid
      call: no tangent pass runs, only the forward.
    * ``"gains"`` in ``wrt`` gives the gain block of ``H p`` in ``gains``' own shape, complex128, in torch's convention for a
      complex leaf (the convention of ``simulate_vis_gain_chi2``'s gradient), following the inputs as the other products
      do; for time-constant gains it is the per-time products added on the host in time order.  ``wrt=None`` appends
      ``"gains"`` when ``d_gains`` is given.  Every other product is its public pass's result for ``vis = G``.
    * ``return_gvis=True`` gives that ``G = conj(m) 2 w U'``, ``m`` the gain product -- NOT ``2 w U'``.
    * The forward V is computed only when ``d_gains`` is given or ``"gains"`` is asked for (one more device block); under
      fixed gains with sky directions and sky products alone the call costs ``simulate_vis_gauss_newton``'s passes.
    * Gains alone do not force the type-3 transform: ``adjoint_path`` and ``force_use_type3`` are honoured when the sky
      part of the call is within fluxes, as for ``simulate_vis_gauss_newton``.

    A gains-only solve against a fixed model is ``simulate_vis_gain_solve``'s: one forward, or a resident ``model=``, and
    the iterations on the device -- here every call reruns the forward.  Not covered: ``model=`` in this call, several
    directions per call, the gradient in the same call (``simulate_vis_gain_chi2``), torch ``hvp``, sharding over GPUs.
    Full 2x2 Jones (leakage) matrices per antenna are ``simulate_vis_jones_gauss_newton``'s."""
    return _gain_gauss_newton(locals(), "gains")


def _gain_gauss_newton(args: dict, kind: str):
    """``simulate_vis_gain_gauss_newton`` (``kind="gains"``) and ``simulate_vis_jones_gauss_newton`` (``kind="jones"``):
    ``args`` is the public function's ``locals()``, ``args[kind]`` its gains or matrices (None: neither,
    ``simulate_vis_gauss_newton``) and ``args["d_" + kind]`` their direction.  The two differ in the blocks the engine's
    pass is given, in the output that receives the product and in the name ``wrt`` has for it."""
    gains, d_gains = args[kind], args["d_" + kind]
    d_fluxes, d_ants, d_baselines, d_radec, d_topo, d_beam_coefs = (
        args[k] for k in ("d_fluxes", "d_ants", "d_baselines", "d_radec", "d_topo", "d_beam_coefs"))
    weights, wrt, quad_per, fluxes, full_stokes = (args[k] for k in ("weights", "wrt", "quad_per", "fluxes", "full_stokes"))
    adjoint_path, beam_coefs, polarized, return_gvis = (
        args[k] for k in ("adjoint_path", "beam_coefs", "polarized", "return_gvis"))
    given = tuple(name for d, name in _GAUSS_NEWTON_NAMES if args[d] is not None)
    if d_gains is not None and gains is None:
        raise ValueError(f"d_{kind} needs {kind}=")
    if kind == "jones" and not polarized:
        raise ValueError("jones needs polarized=True: a 2 x 2 matrix per antenna mixes the two feeds")
    if not given and d_gains is None:
        if gains is not None:
            raise ValueError(f"simulate_vis_{'jones' if kind == 'jones' else 'gain'}_gauss_newton needs a direction: d_fluxes, "
                             f"d_ants, d_baselines, d_radec, d_topo, d_beam_coefs or d_{kind}")
        raise ValueError("simulate_vis_gauss_newton needs a direction: d_fluxes, d_ants, d_baselines, d_radec, d_topo or "
                         "d_beam_coefs")
    if d_ants is not None and d_baselines is not None:
        raise ValueError("give the antenna tangent as d_ants or as d_baselines, not both")
    if d_radec is not None and d_topo is not None:
        raise ValueError("give the source tangent as d_radec or as d_topo, not both")
    if wrt is None:
        wrt = given + ((kind,) if d_gains is not None else ())
    single, names = _fit_keywords(wrt, gains, "quad_per", quad_per, adjoint_path, beam_coefs, polarized, d_beam_coefs, kind=kind)
    run = _describe_run(args)
    run = _own_radec_chain(run, "d_radec" if d_radec is not None else "wrt='radec'", d_radec is not None or "radec" in names,
                           "pass d_topo and ask for wrt='topo', and apply its Jacobian", "pass d_topo and ask for wrt='topo'")
    fluxes, full_stokes = _sky_full_stokes(run, fluxes, full_stokes)
    _host_fluxes(run, fluxes, d_fluxes)
    d_baselines = _baseline_tangent(run, d_ants, d_baselines)
    if d_radec is not None and tuple(d_radec.shape) != (run.nsrc, 2):
        raise ValueError(f"d_radec must have shape ({run.nsrc}, 2), got {tuple(d_radec.shape)}")
    if d_topo is not None and tuple(d_topo.shape) != (run.ntimes, run.nsrc, 3):
        raise ValueError(f"d_topo must have shape ({run.ntimes}, {run.nsrc}, 3), got {tuple(d_topo.shape)}")
    if d_beam_coefs is not None:
        if tuple(d_beam_coefs.shape) != run.beam_coefs.shape:
            raise ValueError(f"d_beam_coefs must be one direction of beam_coefs' shape {run.beam_coefs.shape} (a stack is not "
                             f"covered), got {tuple(d_beam_coefs.shape)}")
        if not (d_beam_coefs.is_complex() if _is_tensor(d_beam_coefs) else np.iscomplexobj(d_beam_coefs)):
            raise ValueError("d_beam_coefs must be complex, like beam_coefs")
    if weights is not None:
        _check_weights(run, weights, "simulate_vis's output")
    gain_block = dgain_block = None
    if gains is not None:
        as_block = _jones_block if kind == "jones" else _gain_block
        gain_block = as_block(run, gains)
        if d_gains is not None:
            if tuple(d_gains.shape) != tuple(gains.shape):
                raise ValueError(f"d_{kind} must have {kind}' shape {tuple(gains.shape)}, got {tuple(d_gains.shape)}")
            if not np.iscomplexobj(_host(d_gains)):
                raise ValueError(f"d_{kind} must be complex, like {kind}")
            if not np.isfinite(_host(d_gains)).all():
                raise ValueError(f"d_{kind} must be finite")
            dgain_block = as_block(run, d_gains)
    hgains = np.zeros(gain_block.shape, dtype=np.complex128) if kind in names else None
    inputs = (d_fluxes, d_ants, d_baselines, d_radec, d_topo, d_beam_coefs, weights)
    dev = _run_device(run, inputs, "a direction or the weights")
    like = next((x for x in inputs + (d_gains,) if _is_tensor(x)), None)
    if d_radec is not None:
        d_topo = np.einsum("tjdc,jc->tjd", _radec_jacobian_of(run), _host(d_radec).astype(np.float64))
    dc = _buffer(run, dev, d_beam_coefs, "complex")
    directions = dict(d_fluxes=None if d_fluxes is None else _host(d_fluxes),
                      d_beam_coefs=None if dc is None else dc.reshape((1,) + run.beam_coefs.shape),
                      d_baselines=_buffer(run, dev, d_baselines, "float64"), d_topo=_buffer(run, dev, d_topo, "float64"))
    buffers = [None if w_ is None else _zeros(dev, w_[0], run.dtype(w_[1])) for w_ in _fit_outputs(run, names, full_stokes)]
    w = None
    if weights is not None:
        w = _host(weights).astype(run.rdt, copy=False) if dev is None or not _is_tensor(weights) or weights.device.type != "cuda" \
            else _on(dev, weights, run.rdt)
    gvis = _gvis_buffer(run, return_gvis)
    _synchronize(dev)
    # (the gains act on the output block whatever path produced it: they do not force the type-3 transform)
    fluxes_only = set(given) <= {"fluxes"} and set(names) <= {"fluxes", kind}
    outputs = dict(zip(("gflux", "gcoefs", "gbls", "gtopo"), buffers), gvis=gvis)
    if gains is None:
        gauss_newton_of = (directions, w, outputs)
    elif kind == "jones":
        gauss_newton_of = (directions, w, dict(outputs, gjones=hgains), ("jones", (gain_block, dgain_block)))
    else:
        gauss_newton_of = (directions, w, dict(outputs, ggains=hgains), (gain_block, dgain_block))
    quad_ft = _engine_simulate(
        run, fluxes, force_use_type3=None if fluxes_only else True, adjoint_path=adjoint_path, gauss_newton_of=gauss_newton_of)
    prods = _fit_gradients(run, single, names, buffers, full_stokes, hgains, gains, like, dev, kind=kind)
    # (no time steps: no rows to add)
    quad = 0.0 if quad_per == "total" and not quad_ft.size else _fit_value(quad_ft, quad_per, like, dev)
    return (quad, prods, _gvis_home(gvis, like, dev)) if return_gvis else (quad, prods)


def simulate_vis_jones_gauss_newton(
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    jones,
    d_fluxes=None,
    d_ants=None,
    d_baselines=None,
    d_radec=None,
    d_topo=None,
    d_beam_coefs=None,
    d_jones=None,
    weights=None,
    wrt=None,
    quad_per: str = "total",
    return_gvis: bool = False,
    adjoint_path: str = "type3",
    beam_coefs=None,
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """``simulate_vis_gauss_newton`` with one 2 x 2 complex matrix per antenna in the data model: the Gauss-Newton product
    of ``simulate_vis_jones_chi2``'s chi2, whose data model is ``V'[x, y] = sum conj(jones[a1][y', y]) jones[a2][x', x]
    V[x', y']``, along a joint direction ``p = (sky directions, d_jones)``, the matrices' block of ``H p`` included.  With
    ``S(X; A, B)[x, y] = sum conj(A[y', y]) B[x', x] X[x', y']`` that product and ``U`` the sky tangent as
    ``simulate_vis_gauss_newton`` defines it, the tangent of the data model is

        ``U' = S(U; J[a1], J[a2]) + S(V; dJ[a1], J[a2]) + S(V; J[a1], dJ[a2])``;

    ``quad = sum w |U'|^2``, ``H = 2 J'^T W J'`` with ``J'`` the Jacobian of V', and ``<p, H p> = 2 quad``, the matrices'
    part of the inner product being ``Re sum conj(d_jones) prod``.  The product is applied on the device to the blocks the
    weighting kernel touches (``fv_sim_jones_weight_block``), whatever path produced them; everything else -- the ``d_*``
    directions, ``weights``, the other names of ``wrt``, ``quad_per``, ``adjoint_path``, ``force_use_type3``, the returned
    tuple -- is ``simulate_vis_gauss_newton``'s.  ``jones[a] = diag(gains[a])`` and ``d_jones[a] = diag(d_gains[a])`` is
    ``simulate_vis_gain_gauss_newton``.

    * Needs ``polarized=True`` (ValueError otherwise).
    * ``jones``: ``simulate_vis_jones_chi2``'s, with its shapes and rules.  ``d_jones``: the direction, ``jones``' own shape
      -- time-constant or per time as ``jones`` is --, complex and finite, or None.  ``d_jones`` alone is a valid call: no
      tangent pass runs, only the forward.
    * ``"jones"`` in ``wrt`` gives the matrices' block of ``H p`` in ``jones``' own shape, complex128, in the convention of
      ``simulate_vis_jones_chi2``'s gradient, following the inputs as the other products do; for time-constant matrices it
      is the per-time products added on the host in time order.  ``wrt=None`` appends ``"jones"`` when ``d_jones`` is given.
      Every other product is its public pass's result for ``vis = G``.
    * ``return_gvis=True`` gives that G, the transposed product applied to ``2 w U'`` -- NOT ``2 w U'`` itself.
    * A weight of 0 flags that one ``(x, y)`` sample; the baseline's other samples still use all four values of U and V.
    * The forward V is computed only when ``d_jones`` is given or ``"jones"`` is asked for (one more device block); the
      device also holds one more fp64 value per visibility of a time block (the rows' terms of quad), which the time
      blocks are sized for.
    * Jones matrices alone do not force the type-3 transform: ``adjoint_path`` and ``force_use_type3`` are honoured when
      the sky part of the call is within fluxes, as for ``simulate_vis_gauss_newton``.

    A matrices-only solve against a fixed model is ``simulate_vis_jones_solve``'s.  Not covered: ``model=`` in this call,
    several directions per call, the gradient in the same call (``simulate_vis_jones_chi2``), torch ``hvp``, sharding over
    GPUs."""
    return _gain_gauss_newton(locals(), "jones")


def _solve_start(run: _Run, gains, per_time: bool):
    """``simulate_vis_gain_solve``'s start: ``gains`` in any of ``simulate_vis_gain_chi2``'s four shapes, or None for ones
    in the shape ``per_time`` chooses.  Returns (the complex128 block (nfreqs, ntimes or 1, nfeed, nant), the gains' own
    shape, whether they are per time)."""
    nant, nfeed = len(run.ants), 2 if run.args["polarized"] else 1
    lead = (nant, 2) if nfeed == 2 else (nant,)
    if gains is None:
        shape = lead + ((run.nfreqs, run.ntimes) if per_time else (run.nfreqs,))
        return np.ones((run.nfreqs, run.ntimes if per_time else 1, nfeed, nant), dtype=np.complex128), shape, bool(per_time)
    _gain_block(run, gains)  # (its checks: complex, one of the four shapes, finite)
    g = _host(gains)
    own = g.ndim == len(lead) + 2
    if per_time and not own:
        raise ValueError(f"per_time=True needs per-time gains of shape {lead + (run.nfreqs, run.ntimes)}, got {g.shape}")
    block = g.reshape(nant, nfeed, run.nfreqs, -1).transpose(2, 3, 1, 0)
    return np.ascontiguousarray(block, dtype=np.complex128), g.shape, own


def _solve_result(block: np.ndarray, shape) -> np.ndarray:
    """An (nfreqs, ntimes or 1, nfeed, nant) block of the solve in the gains' own shape."""
    return np.ascontiguousarray(block.transpose(3, 2, 0, 1)).reshape(shape)


def _jones_solve_start(run: _Run, jones, per_time: bool):
    """``simulate_vis_jones_solve``'s start: ``jones`` in either of ``simulate_vis_jones_chi2``'s shapes, or None for
    identities in the shape ``per_time`` chooses.  Returns (the complex128 block (nfreqs, ntimes or 1, 2, 2, nant), the
    matrices' own shape, whether they are per time)."""
    nant = len(run.ants)
    if jones is None:
        shape = (nant, 2, 2) + ((run.nfreqs, run.ntimes) if per_time else (run.nfreqs,))
        block = np.zeros((run.nfreqs, run.ntimes if per_time else 1, 2, 2, nant), dtype=np.complex128)
        block[:, :, 0, 0] = block[:, :, 1, 1] = 1
        return block, shape, bool(per_time)
    _jones_block(run, jones)  # (its checks: complex, one of the two shapes, finite)
    j = _host(jones)
    own = j.ndim == 5
    if per_time and not own:
        raise ValueError(f"per_time=True needs per-time jones of shape {(nant, 2, 2, run.nfreqs, run.ntimes)}, got {j.shape}")
    block = j.reshape(nant, 2, 2, run.nfreqs, -1).transpose(3, 4, 1, 2, 0)
    return np.ascontiguousarray(block, dtype=np.complex128), j.shape, own


def _jones_solve_result(block: np.ndarray, shape) -> np.ndarray:
    """An (nfreqs, ntimes or 1, 2, 2, nant) block of the solve in the matrices' own shape."""
    return np.ascontiguousarray(block.transpose(4, 2, 3, 0, 1)).reshape(shape)


def _gain_solve(args: dict, kind: str):
    """``simulate_vis_gain_solve`` (``kind="gains"``) and ``simulate_vis_jones_solve`` (``kind="jones"``): ``args`` is the
    caller's ``locals()``, the start came by the keyword ``kind``."""
    jones = kind == "jones"
    start, per_time, weights, model = args[kind], args["per_time"], args["weights"], args["model"]
    data, fluxes, max_iter, tol, ref_ant = args["data"], args["fluxes"], args["max_iter"], args["tol"], args["ref_ant"]
    polarized, precision, device = args["polarized"], args["precision"], args["device"]
    if jones and not polarized:
        raise ValueError("jones needs polarized=True: a 2 x 2 matrix per antenna mixes the two feeds")
    if args["beam_coefs"] is not None and not polarized:  # the forward's message
        raise ValueError(
            "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
        )
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol must be non-negative, got {tol!r}")
    run = _describe_run(args)
    if ref_ant is not None and ref_ant not in run.ants:
        raise ValueError(f"ref_ant must be a key of ants, got {ref_ant!r}")
    if model is None:
        fluxes, _ = _sky_full_stokes(run, fluxes, args["full_stokes"])
    _check_vis_block(run, data, "data")
    if weights is not None:
        _check_weights(run, weights, "data's")
        _run_device(run, (weights,), "weights")
    if model is not None:
        _check_vis_block(run, model, "model")
    block, shape, own_time = (_jones_solve_start if jones else _solve_start)(run, start, per_time)

    import torch

    from . import _lib

    dev = torch.device("cuda", int(device))
    if model is None:
        vis = _engine_simulate(run, fluxes, forward_to=True)
    else:
        vis = _on(dev, model, run.cdt)

    def buffer(x, what):  # as the library reads it: a tensor on the run's device by pointer, anything else as a host array
        if x is None:
            return None
        if _is_tensor(x) and x.device.type == "cuda":
            return _on(x.device, x, run.dtype(what))
        return np.ascontiguousarray(_host(x), dtype=run.dtype(what))

    from .gpu.gpu_simulate import _buffer_addr

    d, w = buffer(data, "complex"), buffer(weights, "real")  # (alive until the call returns)
    (d_ptr, d_dev), (w_ptr, w_dev) = _buffer_addr(d), _buffer_addr(w)
    _synchronize(dev)
    row = {a: i for i, a in enumerate(run.ants)}
    a1 = np.fromiter((row[bl[0]] for bl in run.baselines), np.int32, count=run.nbls)
    a2 = np.fromiter((row[bl[1]] for bl in run.baselines), np.int32, count=run.nbls)
    nunits = (run.nfreqs, run.ntimes) if own_time else (run.nfreqs,)
    niter = np.zeros(1, dtype=np.int32)
    change = np.zeros(nunits, dtype=np.float64)
    chi2 = np.zeros((run.nfreqs, run.ntimes), dtype=np.float64)
    solved = np.zeros(block.shape[:2] + (2, len(run.ants)) if jones else block.shape, dtype=np.int32)
    head = (int(device), int(precision), run.nfreqs, run.ntimes, run.nbls)
    tail = (len(run.ants), _lib.ptr(a1), _lib.ptr(a2), int(own_time), _lib.ptr(vis.data_ptr()), 1, d_ptr, d_dev, w_ptr, w_dev,
            _lib.ptr(block), int(max_iter), float(tol), _lib.ptr(niter), _lib.ptr(change), _lib.ptr(chi2), _lib.ptr(solved))
    if jones:
        _lib.check(_lib.lib().fv_jones_solve(*head, *tail))
    else:
        _lib.check(_lib.lib().fv_gain_solve(*head, 4 if polarized else 1, *tail))
    if ref_ant is not None:  # (feed 0 of the gains, entry [0, 0] of the matrices)
        ref = block[(slice(None), slice(None)) + (0,) * (block.ndim - 3) + (row[ref_ant],)]
        block = block * np.exp(-1j * np.angle(ref)).reshape(ref.shape + (1,) * (block.ndim - 2))
    if jones:  # (both entries of a column alike)
        solved = np.broadcast_to(solved[:, :, None], block.shape)
    result = (_jones_solve_result if jones else _solve_result)
    info = dict(niter=int(niter[0]), converged=bool(niter[0] > 0 and np.all(change < tol)), change=change, chi2=chi2,
                solved=result(solved != 0, shape))
    result = result(block, shape)
    if _is_tensor(data):
        where = data.device if data.device.type == "cuda" else None
        result = torch.from_numpy(result).to(where or "cpu")
        info.update({k: torch.from_numpy(np.ascontiguousarray(info[k])).to(where or "cpu") for k in ("change", "chi2", "solved")})
    return (result, info, vis) if args["return_model"] else (result, info)


def simulate_vis_gain_solve(
    data,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    gains=None,
    per_time: bool = False,
    weights=None,
    model=None,
    return_model: bool = False,
    max_iter: int = 100,
    tol: float = 1e-8,
    ref_ant=None,
    beam_coefs=None,
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Sky-based gain calibration on the device: the per-antenna gains that minimise ``simulate_vis_gain_chi2``'s
    ``chi2 = sum w |conj(g[a1]) g[a2] V - data|^2`` for a FIXED model ``V = simulate_vis(ants, fluxes, ra, dec, ...)``.  V does
    not depend on the gains, so one call runs the forward once -- or takes a resident ``model=`` -- and then iterates on the
    device block (``fv_gain_solve``): for fixed V the problem in one antenna's gain, the others held, is linear, and the
    alternating per-antenna solve (StefCal; Salvini & Wijnholds 2014) sets ``g^ = num / den`` from the normal sums
    ``num = sum w g[other] V conj(d)`` (the conjugate for the second antenna of a pair), ``den = sum w |g[other]|^2 |V|^2``,
    taking ``g^`` on odd iterations and ``(g^ + g) / 2`` on even ones.  Returns ``(gains, info)``, with ``return_model=True``
    ``(gains, info, model)``.

    * ``data``, ``weights``: ``simulate_vis_gain_chi2``'s, numpy arrays or tensors, tensors on the run's device read by
      pointer.  A sample is used when its weight is positive and it is no auto-correlation: autos are quadratic in one gain
      and count as flagged throughout, in the update and in the reported chi2.  A flagged datum is not read.  A negative or
      non-finite weight, a non-finite datum at a used sample and a non-finite model value fail the call.
    * ``gains``: the start, in any of ``simulate_vis_gain_chi2``'s four shapes; its shape decides between time-constant and
      per-time gains.  None starts from ones, time-constant or, with ``per_time=True``, per time.  ``per_time=True`` with
      time-constant ``gains`` is a ValueError.  For time-constant gains the normal sums are added over the times in
      ascending order and one gain serves all times.  The result has the start's shape, is complex128 whatever
      ``precision`` is, and follows ``data`` as the other outputs do.
    * ``model``: None runs the forward of the same arguments into a device tensor of ``simulate_vis``'s output shape, by
      whatever path ``simulate_vis`` would take (gains force nothing), with ``beam_coefs`` through basis beams.  A tensor on
      the run's device is used where it lies, a host array is uploaded once; no forward runs and ``fluxes`` may be None.
      ``return_model=True`` appends the device tensor, so that a later call on new data, new weights or new start gains
      costs no forward.
    * ``max_iter``, ``tol``: a solve unit is a frequency for time-constant gains and a (frequency, time) for per-time gains;
      per unit ``change = max |g_new - g| / max |g_new|``.  The loop ends after the first iteration at which every unit has
      ``change < tol``, or at ``max_iter``; every unit iterates until then.  ``tol=0`` runs exactly ``max_iter`` iterations.
    * ``ref_ant``: a key of ``ants``.  The common phase of a unit is not constrained by the data and is left where the
      iteration puts it; with ``ref_ant`` each unit's gains, both feeds alike, are multiplied at the end by
      ``exp(-i arg g[ref_ant, feed 0])``.  chi2 does not change.
    * ``info``: ``niter``; ``converged``; ``change`` per unit, ``(nfreqs,)`` or ``(nfreqs, ntimes)``; ``chi2``, the
      ``(nfreqs, ntimes)`` float64 array of ``sum w |V' - data|^2`` over the used samples at the returned gains; ``solved``,
      a bool array in ``gains``' shape, False where an antenna had no used sample (it keeps its start value).
    * Polarized runs: with cross-hand model visibilities the phase between the feeds is barely constrained and the
      iteration converges very slowly (the tests' case of 8 antennas with cross-hands at 10 % of the parallel hands still
      changes by 1.8e-5 after 200 iterations and by 5.4e-7 after 400).  Flag the cross-hands (weight 0) to solve each feed
      on its parallel hand, as calibration packages do: the feeds decouple and the same case reaches 1e-10 in 56 iterations.
    * With the default ``baselines=None`` there is one baseline per redundant group and the gains are those of each group's
      representative pair: a calibration passes explicit ``baselines``.

    Every other keyword means what it means for ``simulate_vis``.  Not differentiable, and no torch operation.  Full 2 x 2
    Jones (leakage) matrices, which use the cross-hands, are ``simulate_vis_jones_solve``'s.  Not covered: a joint sky and
    gain solve (the CG loop over ``simulate_vis_gain_gauss_newton``), ``model=`` in ``simulate_vis_gain_chi2`` and
    ``simulate_vis_gain_gauss_newton``, sharding over GPUs."""
    return _gain_solve(locals(), "gains")


def simulate_vis_jones_solve(
    data,
    ants: dict,
    fluxes,
    ra: np.ndarray,
    dec: np.ndarray,
    freqs: np.ndarray,
    times,
    beam,
    telescope_loc,
    *,
    jones=None,
    per_time: bool = False,
    weights=None,
    model=None,
    return_model: bool = False,
    max_iter: int = 100,
    tol: float = 1e-8,
    ref_ant=None,
    beam_coefs=None,
    full_stokes: bool = None,
    beam_idx: np.ndarray = None,
    baselines: list = None,
    precision: int = 2,
    polarized: bool = False,
    eps: float = None,
    upsample_factor=2,
    beam_spline_opts: dict = None,
    use_feed: str = "x",
    flat_array_tol: float = 1e-6,
    interpolation_function: str = "az_za_map_coordinates",
    nprocesses: int | None = 1,
    nthreads: int | None = None,
    coord_method: str = "CoordinateRotationERFA",
    coord_method_params: dict | None = None,
    force_use_type3: bool = False,
    force_use_ray: bool = False,
    trace_mem: bool = False,
    backend: str = "gpu",
    max_memory=np.inf,
    min_chunks: int = 1,
    source_buffer=1.0,
    device: int = 0,
    coord_mgr=None,
    reference_compat: bool = True,
    astrom: np.ndarray = None,
    device_astrometry: bool = False,
):
    """Sky-based polarized calibration on the device: the 2 x 2 matrix per antenna -- the two gains and the leakage between
    the feeds (D-terms) -- that minimises ``simulate_vis_jones_chi2``'s ``chi2 = sum w |V' - data|^2``,

        ``V'[x, y] = sum_{x', y'} conj(jones[a1][y', y]) jones[a2][x', x] V[x', y']``,

    for a FIXED model ``V = simulate_vis(ants, fluxes, ra, dec, ..., polarized=True)``.  ``simulate_vis_gain_solve`` with
    matrices in place of gains: one forward, or a resident ``model=``, and then the alternating per-antenna solve on the
    device block (``fv_jones_solve``; StefCal for full Jones matrices, Salvini & Wijnholds 2014, section 5).  For fixed V the
    problem in one antenna's matrix, the others held, is linear and splits into one 2 x 2 Hermitian system ``A x = b`` per
    measured feed (column ``jones[a][:, c]``); the solve takes ``A^-1 b`` on odd iterations and its mean with the previous
    iterate on even ones.  Unlike the diagonal solve it uses the cross-hands.  Returns ``(jones, info)``, with
    ``return_model=True`` ``(jones, info, model)``.

    * Needs ``polarized=True`` (ValueError otherwise).
    * ``data``, ``weights``, ``model``, ``return_model``, ``max_iter``, ``tol``: ``simulate_vis_gain_solve``'s, with the same
      rules for tensors on the run's device, the same units (a frequency, or a (frequency, time) for per-time matrices)
      and the same failures for a negative or non-finite weight, a non-finite datum at a used sample and a non-finite
      model value.  A sample is used when its weight is positive and it is no auto-correlation; a weight of 0 flags that
      one ``(x, y)`` sample and the baseline's other samples still use all four model values.
    * ``jones``: the start, ``(nant, 2, 2, nfreqs)`` or per time ``(nant, 2, 2, nfreqs, ntimes)`` as
      ``simulate_vis_jones_chi2`` takes it; its shape decides between time-constant and per-time matrices.  None starts
      from identities, time-constant or, with ``per_time=True``, per time.  ``per_time=True`` with time-constant ``jones``
      is a ValueError.  The result has the start's shape, is complex128 whatever ``precision`` is, and follows ``data``.
    * Rank rule: a column is solved when ``A00 > 0``, ``A11 > 0`` and ``det A > 2^-30 A00 A11``; otherwise both of its
      entries keep their values.  A column with a single used sample is rank one, and so is every column when the model
      is diagonal (no cross-hand power) and the cross-hands are flagged: then nothing is solved, and that case is
      ``simulate_vis_gain_solve``'s.
    * ``ref_ant``: a key of ``ants``.  With it each unit's matrices are multiplied at the end by
      ``exp(-i arg jones[ref_ant][0, 0])``; chi2 does not change.  For an unpolarized model (V proportional to the
      identity on every baseline) the data also leave a common unitary factor free, ``jones[a] -> jones[a] U``: it stays
      where the iteration puts it.
    * ``info``: ``niter``; ``converged``; ``change`` per unit, ``max |new - old| / max |new|`` over the unit's ``4 nant``
      entries; ``chi2``, the ``(nfreqs, ntimes)`` float64 array over the used samples at the returned matrices;
      ``solved``, a bool array in ``jones``' shape, both entries of a column alike.
    * Speed: with a model whose cross-hands are as strong as its parallel hands the tests' case of 8 antennas reaches
      ``tol=1e-10`` in 46 to 52 iterations.  With cross-hands at 10 % of the parallel hands the leakage terms are barely
      constrained and the iteration is slow: the same case still changes by 7e-8 to 2e-5 at iteration 400, depending
      on the seed (``tests/test_jones_solve_host.py``).
    * With the default ``baselines=None`` there is one baseline per redundant group and the matrices are those of each
      group's representative pair: a calibration passes explicit ``baselines``.

    Every other keyword means what it means for ``simulate_vis``.  Not differentiable, and no torch operation.  Not covered:
    a joint sky and Jones solve (the CG loop over ``simulate_vis_jones_gauss_newton``), ``model=`` in the chi2 and
    Gauss-Newton calls, sharding over GPUs."""
    return _gain_solve(locals(), "jones")
