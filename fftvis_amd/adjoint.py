"""Adjoint of ``simulate_vis`` with respect to ``fluxes``, and a torch autograd entry point.

``simulate_vis`` is linear in ``fluxes``: V = A F.  The adjoint is taken for the REAL inner products

    Re <A F, G> = <F, A^T G>      for every real F and complex G,

because the map is real-linear, not complex-linear (flipped two-beam baselines are conjugated, fluxes are real Stokes
parameters).  ``A^T G`` has the shape of ``fluxes``.  The device computes it per (time, frequency group, beam pair)
with the roles of the forward's type-3 transform swapped (``fv_sim_run_adjoint``, DESIGN.md "Adjoint").
"""

from __future__ import annotations

import numpy as np

from .core.beams import feed_index
from .core.coords import julian_dates
from .core.simulate import default_accuracy_dict
from .core.utils import get_pos_reds, validate_beam_idx


def _is_tensor(x) -> bool:
    import sys

    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


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
):
    """``A^T vis``: the transpose of ``simulate_vis``'s map from ``fluxes`` to visibilities, for the same arguments.

    ``vis`` has ``simulate_vis``'s output shape -- (nfreqs, ntimes, nbls), polarized (nfreqs, ntimes, 2, 2, nbls) -- as a
    numpy array or as a torch tensor on the run's device (handed to the library by pointer, no host copy).  The result
    F satisfies Re <simulate_vis(fluxes), vis> = <fluxes, F> for every real ``fluxes`` and has their shape: (nsrc, nfreqs)
    for Stokes I, (nsrc, nfreqs, 4) with ``full_stokes=True`` (polarized runs only); real, of the run's precision,
    numpy for numpy input and a tensor on ``vis``' device for a tensor.  Every other keyword means what it means for
    ``simulate_vis``, ``reference_compat`` included; on lattice arrays, where ``simulate_vis`` takes the type-1 transform,
    the adjoint uses the type-3 transform (both compute the same map to ``eps``).  Sources below the horizon at every
    time get exactly 0.  Not covered: ``beam_coefs`` (NotImplementedError), a sharded multi-GPU adjoint.
    """
    if beam_coefs is not None:
        raise NotImplementedError("simulate_vis_adjoint does not support basis beams (beam_coefs)")
    if backend != "gpu":
        raise ValueError(f"Unsupported backend: {backend}")
    if full_stokes and not polarized:
        raise ValueError("full_stokes=True needs polarized=True (a full-Stokes sky needs a polarized simulation)")
    if eps is None:
        eps = default_accuracy_dict[precision]
    ants = {k: np.array(v) for k, v in ants.items()}
    beam_list = list(beam) if isinstance(beam, (list, tuple)) else [beam]
    beam_idx = validate_beam_idx(beam_idx, beam_coefs, len(beam_list), len(ants))
    feed_index(use_feed)
    if baselines is None:
        baselines = [red[0] for red in get_pos_reds(ants, include_autos=True)]
    nsrc = int(np.size(ra))
    nfreqs = int(np.size(freqs))
    ntimes = len(julian_dates(times))
    nbls = len(baselines)
    want = (nfreqs, ntimes, 2, 2, nbls) if polarized else (nfreqs, ntimes, nbls)
    if tuple(vis.shape) != want:
        raise ValueError(f"vis must have simulate_vis's output shape {want}, got {tuple(vis.shape)}")
    rdt = np.float32 if precision == 1 else np.float64
    cdt = np.complex64 if precision == 1 else np.complex128
    on_device = _is_tensor(vis) and vis.device.type == "cuda"
    if on_device:
        import torch

        if (vis.device.index or 0) != int(device):
            raise ValueError(f"vis lives on {vis.device}, the run is on cuda:{int(device)}")
        tc = torch.complex64 if precision == 1 else torch.complex128
        g = vis.detach().to(tc).resolve_conj().resolve_neg()  # (a lazily conjugated view's memory is not G)
        gflux = torch.zeros((nsrc, nfreqs, 2, 2) if full_stokes else (nsrc, nfreqs),
                            dtype=tc if full_stokes else (torch.float32 if precision == 1 else torch.float64),
                            device=vis.device)
        torch.cuda.synchronize(vis.device)  # the library's streams do not follow torch's: g and gflux are complete
    else:
        g = vis.detach().resolve_conj().resolve_neg().cpu().numpy() if _is_tensor(vis) else vis
        g = np.asarray(g).astype(cdt, copy=False)
        gflux = np.zeros((nsrc, nfreqs, 2, 2) if full_stokes else (nsrc, nfreqs), dtype=cdt if full_stokes else rdt)
    # the catalog's shape is all the engine needs of the fluxes
    fluxes = np.zeros((nsrc, nfreqs, 4) if full_stokes else (nsrc, nfreqs), dtype=rdt)

    from .wrapper import create_simulation_engine, device_chunks

    nax = nfeed = 2 if polarized else 1
    engine = create_simulation_engine(backend=backend, device=device)
    nchunks = device_chunks(device, max_memory, min_chunks, beam_list, nax, nfeed, len(ants), nsrc, precision,
                            source_buffer, nfreqs)
    gc = engine.simulate(
        ants=ants, freqs=np.asarray(freqs), fluxes=fluxes, beam_list=beam_list, beam_idx=beam_idx,
        ra=ra, dec=dec, times=times, telescope_loc=telescope_loc, baselines=baselines,
        precision=precision, polarized=polarized, eps=eps, upsample_factor=upsample_factor,
        beam_spline_opts=beam_spline_opts, flat_array_tol=flat_array_tol,
        interpolation_function=interpolation_function, nprocesses=nprocesses, nthreads=nthreads,
        coord_method=coord_method, coord_method_params=coord_method_params,
        force_use_type3=force_use_type3, force_use_ray=force_use_ray, trace_mem=trace_mem,
        nchunks=nchunks, source_buffer=source_buffer, coord_mgr=coord_mgr, use_feed=use_feed,
        reference_compat=reference_compat, astrom=astrom, device_astrometry=device_astrometry,
        adjoint_of=(g, gflux),
    )
    out = stokes_adjoint(gc, full_stokes)
    if _is_tensor(vis) and not on_device:  # a host tensor in, a host tensor out
        import torch

        return torch.from_numpy(np.ascontiguousarray(out))
    return out


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


def _autograd_function():
    import torch

    class _SimulateVis(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fluxes, kwargs):
            from .wrapper import simulate_vis

            ctx.kwargs = kwargs
            ctx.full_stokes = fluxes.ndim == 3
            ctx.flux_dtype = fluxes.dtype
            vis = simulate_vis(fluxes=fluxes.detach().cpu().numpy(), **kwargs)
            return torch.from_numpy(np.ascontiguousarray(vis)).to(fluxes.device)

        @staticmethod
        def backward(ctx, grad_output):
            if not ctx.needs_input_grad[0]:
                return None, None
            g = simulate_vis_adjoint(grad_output, full_stokes=ctx.full_stokes, **ctx.kwargs)
            if not _is_tensor(g):
                g = torch.from_numpy(g)
            return g.to(device=grad_output.device, dtype=ctx.flux_dtype), None

    return _SimulateVis


_FN = None


def torch_simulate_vis(fluxes, **kwargs):
    """``simulate_vis`` as a differentiable torch operation of ``fluxes`` (a real tensor, (nsrc, nfreqs) or
    (nsrc, nfreqs, 4)); every other argument is a keyword of ``simulate_vis`` (``ants``, ``ra``, ``dec``, ``freqs``,
    ``times``, ``beam``, ``telescope_loc``, ...).  Returns the visibilities as a complex tensor on ``fluxes``' device.
    The backward pass is ``simulate_vis_adjoint`` of the incoming gradient: under torch's convention for a real input
    and a complex output the gradient is Re(A^H g), the adjoint defined there."""
    global _FN
    if _FN is None:
        _FN = _autograd_function()
    if kwargs.get("beam_coefs") is not None:
        raise NotImplementedError("torch_simulate_vis does not support basis beams (beam_coefs)")
    return _FN.apply(fluxes, kwargs)
