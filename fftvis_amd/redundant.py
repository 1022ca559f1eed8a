"""Redundant-baseline calibration on the device ("Redundant solve"): the per-antenna gains together with one
unknown visibility per redundant group, without a sky model.

The data model is ``V'[f, t, pol, k] = conj(g[p, a1]) g[q, a2] U[f, t, pol, group[k]]``.  ``redundant_groups`` builds the
groups, ``redundant_firstcal`` finds the start of data with cable delays (``fv_firstcal_pair_delays``,
``fv_firstcal_offsets``), ``redundant_gain_solve`` alternates the two linear halves on a device block (``fv_redundant_solve``),
``redundant_average`` is the visibility half alone (``fv_redundant_vis_rows``), ``redundant_abscal`` fits what the data leave
free to a model of the group visibilities (``fv_abscal_slopes``) and ``fix_redundant_degeneracies`` brings it to a
reference's gains.  The host layer (shapes of the gains, their start, device buffers) is the gain solve's, in
``adjoint``.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from .adjoint import (
    _Run,
    _check_vis_block,
    _check_weights,
    _gain_block,
    _host,
    _is_tensor,
    _on,
    _run_device,
    _solve_result,
    _solve_start,
    _synchronize,
)
from .core.utils import get_pos_reds


def redundant_groups(ants: dict, baselines: list = None, decimals: int = 3):
    """The redundant groups of an array and the group of every baseline: ``(reds, baselines, group)``.

    * ``reds``: ``get_pos_reds(ants, decimals, include_autos=False)``, a list of lists of antenna pairs, every pair in the
      orientation its group measures.
    * ``baselines``: None means every baseline, in group order (``[bl for red in reds for bl in red]``): a group's baselines
      are then consecutive, which is what the kernels read fastest.  A list is taken as it stands.
    * ``group``: int32, the index into ``reds`` of every baseline.

    A listed baseline that appears in its group only with the opposite orientation is a ValueError: swap the pair and
    conjugate the datum (transposing ``[x, y]`` when polarized) -- the kernels carry no flip.  An auto-correlation in
    ``baselines`` gets a group of its own, appended to ``reds``, and counts as flagged."""
    return _groups(ants, None, baselines, decimals)


def _groups(ants, reds, baselines, decimals=3):
    reds = [list(map(tuple, red)) for red in (get_pos_reds(ants, decimals, include_autos=False) if reds is None else reds)]
    if baselines is None:  # group order: nothing to look up
        group = np.repeat(np.arange(len(reds), dtype=np.int32), [len(red) for red in reds])
        return reds, [bl for red in reds for bl in red], group
    index = {bl: r for r, red in enumerate(reds) for bl in red}
    baselines = [tuple(bl) for bl in baselines]
    group = np.zeros(len(baselines), dtype=np.int32)
    for k, (i, j) in enumerate(baselines):
        if i not in ants or j not in ants:
            raise ValueError(f"baseline {(i, j)} names an antenna that is not a key of ants")
        if (i, j) not in index:
            if i == j:
                index[(i, j)] = len(reds)
                reds.append([(i, j)])
            elif (j, i) in index:
                raise ValueError(
                    f"baseline {(i, j)} is in its redundant group as {(j, i)}: swap the pair and conjugate the datum "
                    "(transposing [x, y] when polarized); the kernels carry no flip"
                )
            else:
                raise ValueError(f"baseline {(i, j)} is in no redundant group")
        group[k] = index[(i, j)]
    return reds, baselines, group


def _block_run(data, ants, polarized, precision, device) -> _Run:
    """What the gain solve's host layer reads of a run, from a data block instead of a simulation's arguments."""
    if precision not in (1, 2):
        raise ValueError(f"precision must be 1 or 2, got {precision!r}")
    tail = 3 if polarized else 1
    shape = tuple(data.shape)
    if len(shape) != 2 + tail or (polarized and shape[2:4] != (2, 2)):
        want = "(nfreqs, ntimes, 2, 2, nbls)" if polarized else "(nfreqs, ntimes, nbls)"
        raise ValueError(f"data must have shape {want}, got {shape}")
    return _Run(
        args=dict(polarized=bool(polarized), device=device, precision=precision), ants={k: np.array(v) for k, v in ants.items()},
        beam_list=None, beam_idx=None, beam_coefs=None, baselines=None, eps=None, astrom=None, nsrc=0, nfreqs=shape[0],
        ntimes=shape[1], nbls=shape[-1], rdt=np.float32 if precision == 1 else np.float64,
        cdt=np.complex64 if precision == 1 else np.complex128, vis_shape=shape,
    )


def _block_inputs(run: _Run, ants, reds, baselines, data, weights):
    """The checks and the buffers both entry points share: (reds, baselines, group, a1, a2, d, w and their addresses)."""
    reds, baselines, group = _groups(ants, reds, baselines)
    if len(baselines) != run.nbls:
        raise ValueError(f"data holds {run.nbls} baselines, baselines lists {len(baselines)}")
    _check_vis_block(run, data, "data")
    if weights is not None:
        _check_weights(run, weights, "data's")
        _run_device(run, (weights,), "weights")
    row = {a: i for i, a in enumerate(run.ants)}
    a1 = np.fromiter((row[bl[0]] for bl in baselines), np.int32, count=run.nbls)
    a2 = np.fromiter((row[bl[1]] for bl in baselines), np.int32, count=run.nbls)
    return reds, baselines, group, a1, a2


def _buffer(run: _Run, x, what):
    """As the library reads it: a tensor on the run's device by pointer, anything else as a host array."""
    if x is None:
        return None
    if _is_tensor(x) and x.device.type == "cuda":
        return _on(x.device, x, run.dtype(what))
    return np.ascontiguousarray(_host(x), dtype=run.dtype(what))


def _follow(data, **arrays):
    """Outputs follow ``data``: tensors where it is a tensor, on its device."""
    if not _is_tensor(data):
        return arrays
    import torch

    where = data.device if data.device.type == "cuda" else "cpu"
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(where) for k, v in arrays.items()}


def redundant_gain_solve(
    data,
    ants: dict,
    *,
    reds: list = None,
    baselines: list = None,
    gains=None,
    per_time: bool = False,
    weights=None,
    max_iter: int = 200,
    tol: float = 1e-8,
    ref_ant=None,
    polarized: bool = False,
    precision: int = 2,
    device: int = 0,
):
    """Redundant calibration on the device: the per-antenna gains ``g`` and one visibility ``U`` per redundant group that
    minimise ``chi2 = sum w |conj(g[a1]) g[a2] U[group] - data|^2``, without a sky model (``fv_redundant_solve``).  The two
    halves are linear and alternate on a block that stays on the device: for fixed gains ``U = sum w conj(m) d / sum w |m|^2``
    over a group's used samples, ``m = conj(g[a1]) g[a2]`` (``redundant_average``); for fixed ``U`` the gains are
    ``simulate_vis_gain_solve``'s with the model ``V[k] = U[group[k]]`` and its update: ``g^ = num / den``, taken on odd
    iterations and averaged with ``g`` on even ones.  ``U`` starts from 0.  Returns ``(gains, vis, info)``.

    * ``data``, ``weights``: ``simulate_vis``'s block over ``baselines``, ``(nfreqs, ntimes, nbls)`` or, polarized,
      ``(nfreqs, ntimes, 2, 2, nbls)``; numpy arrays or tensors, a tensor on the run's device is read by pointer.  A sample
      is used when its weight is positive and it is no auto-correlation; a flagged datum is not read.  A negative or
      non-finite weight and a non-finite datum at a used sample fail the call.
    * ``reds``, ``baselines``: ``redundant_groups``'; ``reds=None`` groups ``ants`` by position, ``baselines=None`` means
      every baseline in group order.
    * ``gains``, ``per_time``, ``max_iter``, ``tol``, ``ref_ant``: ``simulate_vis_gain_solve``'s -- the start in any of its
      four shapes or None for ones, the shape rule, the solve units, the end of the loop and the reference antenna.
    * ``vis``: complex128 ``(nfreqs, ntimes, ngroups)`` or ``(nfreqs, ntimes, 2, 2, ngroups)``, the layout of
      ``simulate_vis(..., baselines=[red[0] for red in reds])``; per time even for time-constant gains; from one more
      visibility step at the returned gains (before ``ref_ant``, which does not change ``conj(g[a1]) g[a2]``).
    * ``info``: ``niter``, ``converged``, ``change``, ``chi2`` ``(nfreqs, ntimes)`` at the returned gains and visibilities,
      ``solved`` in the gains' shape, ``vis_solved`` in ``vis``' shape (False where a group had no used sample: its ``vis`` is
      0), ``reds`` and ``baselines`` as used.
    * The data leave four things free per solve unit and feed -- amplitude, phase and a phase gradient across the array --
      and the result has them wherever the iteration left them: ``redundant_abscal`` (against a model of the group
      visibilities) or ``fix_redundant_degeneracies`` (against reference gains).
    * Convergence (numpy prototype, unit start, ``tol=1e-10``, noiseless): hex-19, hex-37 and a 4 x 4 grid with gain errors
      of 5-20 % take 40-56 iterations; small arrays are slower (hex-7: 190-260, 3 x 3 grid: 120-190).  Polarized with
      cross-hands as strong as the parallel hands 52-54, with the cross-hands flagged 74-84; weak cross-hands that are USED
      (10 %) take over a thousand: flag them, as for ``simulate_vis_gain_solve``.

    Outputs follow ``data`` to its device.  Not differentiable.  A start within a phase wrap of the truth -- firstcal, for
    data whose gains carry cable delays -- is ``redundant_firstcal``'s ``gains``.  Not covered: Jones matrices, a joint sky
    and redundant solve, near-redundancy, sharding over GPUs; the degeneracies against a sky model are ``redundant_abscal``'s."""
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol must be non-negative, got {tol!r}")
    run = _block_run(data, ants, polarized, precision, device)
    if ref_ant is not None and ref_ant not in run.ants:
        raise ValueError(f"ref_ant must be a key of ants, got {ref_ant!r}")
    reds, baselines, group, a1, a2 = _block_inputs(run, ants, reds, baselines, data, weights)
    block, shape, own_time = _solve_start(run, gains, per_time)

    import torch

    from . import _lib
    from .gpu.gpu_simulate import _buffer_addr

    d, w = _buffer(run, data, "complex"), _buffer(run, weights, "real")  # (alive until the call returns)
    (d_ptr, d_dev), (w_ptr, w_dev) = _buffer_addr(d), _buffer_addr(w)
    _synchronize(torch.device("cuda", int(device)))
    tpol, ngroups = 4 if polarized else 1, len(reds)
    niter = np.zeros(1, dtype=np.int32)
    change = np.zeros((run.nfreqs, run.ntimes) if own_time else (run.nfreqs,), dtype=np.float64)
    chi2 = np.zeros((run.nfreqs, run.ntimes), dtype=np.float64)
    solved = np.zeros(block.shape, dtype=np.int32)
    uvis = np.zeros((run.nfreqs, run.ntimes, tpol, ngroups), dtype=np.complex128)
    vis_solved = np.zeros(uvis.shape, dtype=np.int32)
    _lib.check(_lib.lib().fv_redundant_solve(
        int(device), int(precision), run.nfreqs, run.ntimes, run.nbls, tpol, len(run.ants), _lib.ptr(a1), _lib.ptr(a2), ngroups,
        _lib.ptr(group), int(own_time), d_ptr, d_dev, w_ptr, w_dev, _lib.ptr(block), _lib.ptr(uvis), int(max_iter), float(tol),
        _lib.ptr(niter), _lib.ptr(change), _lib.ptr(chi2), _lib.ptr(solved), _lib.ptr(vis_solved)))
    if ref_ant is not None:  # (feed 0's phase, both feeds alike)
        ref = block[:, :, 0, list(run.ants).index(ref_ant)]
        block = block * np.exp(-1j * np.angle(ref))[:, :, None, None]
    out = _follow(data, gains=_solve_result(block, shape), vis=uvis.reshape(run.vis_shape[:-1] + (ngroups,)), change=change,
                  chi2=chi2, solved=_solve_result(solved != 0, shape), vis_solved=(vis_solved != 0).reshape(run.vis_shape[:-1] + (ngroups,)))
    info = dict(niter=int(niter[0]), converged=bool(niter[0] > 0 and np.all(change < tol)), change=out["change"], chi2=out["chi2"],
                solved=out["solved"], vis_solved=out["vis_solved"], reds=reds, baselines=baselines)
    return out["gains"], out["vis"], info


def _firstcal_pairs(group):
    """Consecutive members of every group in ascending baseline index: two int32 arrays of nbls - (groups with members)
    baseline indices.  They span every within-group difference."""
    order = np.argsort(group, kind="stable")
    same = group[order][1:] == group[order][:-1]
    return order[:-1][same].astype(np.int32), order[1:][same].astype(np.int32)


def redundant_firstcal(
    data,
    ants: dict,
    freqs,
    *,
    reds: list = None,
    baselines: list = None,
    weights=None,
    offsets=None,
    pad: int = 8,
    max_iter: int = 200,
    tol: float = 1e-8,
    ref_ant=None,
    polarized: bool = False,
    precision: int = 2,
    device: int = 0,
):
    """Firstcal on the device: the start ``redundant_gain_solve`` needs on data whose gains carry cable delays.  The model is
    one delay and one complex number per antenna and feed, constant in time: ``g[a](nu) = c[a] exp(2 pi i tau[a] (nu -
    mean(freqs)))``.  Returns ``(gains, vis, info)``; ``redundant_gain_solve(data, ants, gains=gains, ...)`` then converges in a
    few iterations, and every channel lands on the same smooth value of the degeneracies, so that
    ``fix_redundant_degeneracies`` applies.

    * Stage 1, delays (``fv_firstcal_pair_delays``).  For two baselines ``k = (i, j)``, ``k' = (m, n)`` of one redundant group
      the group's visibility cancels out of ``z[f] = sum_t d[k] conj(d[k'])``, whose phase winds with the delay
      ``tau_j - tau_i - tau_n + tau_m``.  The pairs are consecutive members of every group (``nbls - ngroups`` of them);
      polarized data use the parallel hands, feed p reads ``[p, p]``; weights act as flags here.  The delay of a pair is the
      peak of ``|sum_f z[f] exp(-2 pi i n f / ND)|^2`` over ``ND = pad nfreqs`` bins, refined by four rounds of a parabola
      through three points of the exact periodogram at half-widths 1, 1/4, 1/16 and 1/64 of a bin.  A pair is used when at
      least two channels have a non-zero ``z``.  The antenna delays are the minimum-norm least-squares solution of the used
      pairs' equations (``lstsq``, on the host: the work is nant-sized), so the common delay and the delay gradient across
      the array, which the data leave free, are 0.  Pair delays beyond ``+-1 / (2 dnu)`` alias.
    * Stage 2, one number per antenna (``fv_firstcal_offsets``).  The block is derotated by the delay model into a buffer of
      the call and ``redundant_gain_solve``'s iteration runs on it with the whole block as one solve unit: ``max_iter``,
      ``tol`` and the messages of bad input are its.  ``offsets``: the start, ``(nant,)`` or ``(nant, 2)`` complex, None for ones.
    * ``data``, ``weights``, ``reds``, ``baselines``, ``polarized``, ``precision``, ``device``, ``ref_ant``:
      ``redundant_gain_solve``'s; ``freqs``: ``(nfreqs,)`` in Hz, at least two, uniformly spaced (to 1e-6 of the spacing).
    * ``gains``: complex128 ``(nant, nfreqs)`` or ``(nant, 2, nfreqs)``; ``vis``: the group visibilities at these gains in
      ``redundant_gain_solve``'s layout.
    * ``info``: ``delays`` ``(nant[, 2])`` in seconds, ``offsets`` (the ``c[a]``), ``pairs`` (a list of baseline pairs),
      ``pair_delays`` and ``pair_used`` ``([2,] npairs)``, ``niter``, ``converged``, ``change``, ``chi2`` ``(nfreqs, ntimes)``,
      ``solved`` ``(nant[, 2])`` (False for an antenna in no used pair, whose delay is 0, or without a used sample),
      ``vis_solved``, ``reds`` and ``baselines`` as used.

    Outputs follow ``data`` to its device.  Not differentiable.  Not covered: polarity flips (pi offsets of swapped feeds),
    per-time delays, non-uniform channels, aliasing beyond ``+-1 / (2 dnu)``, Jones matrices, sharding over GPUs; the
    amplitude and the phase gradient the data leave free are ``redundant_abscal``'s."""
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol must be non-negative, got {tol!r}")
    run = _block_run(data, ants, polarized, precision, device)
    nu = np.asarray(_host(freqs), dtype=np.float64)
    if nu.shape != (run.nfreqs,):
        raise ValueError(f"freqs must have shape ({run.nfreqs},), got {nu.shape}")
    if run.nfreqs < 2:
        raise ValueError("firstcal needs at least two channels")
    dnu = (nu[-1] - nu[0]) / (run.nfreqs - 1)
    if not (np.isfinite(dnu) and dnu != 0.0 and np.all(np.abs(np.diff(nu) - dnu) <= 1e-6 * abs(dnu))):
        raise ValueError("freqs must be uniformly spaced (to 1e-6 of the spacing)")
    if int(pad) != pad or pad < 1 or pad * run.nfreqs >= 1 << 20:
        raise ValueError(f"pad must be a positive integer with pad * nfreqs < 2**20, got {pad!r}")
    if ref_ant is not None and ref_ant not in run.ants:
        raise ValueError(f"ref_ant must be a key of ants, got {ref_ant!r}")
    reds, baselines, group, a1, a2 = _block_inputs(run, ants, reds, baselines, data, weights)
    nant, nfeed = len(run.ants), 2 if polarized else 1
    lead = (nant, 2) if polarized else (nant,)
    if offsets is None:
        c = np.ones((nfeed, nant), dtype=np.complex128)
    else:
        c = _host(offsets)
        if not np.iscomplexobj(c) or c.shape != lead:
            raise ValueError(f"offsets must be complex of shape {lead}, got {c.shape}")
        if not np.isfinite(c).all():
            raise ValueError("offsets must be finite")
        c = np.array(c.reshape(nant, nfeed).T, dtype=np.complex128, order="C")  # a copy: the library writes the result into it
    pair1, pair2 = _firstcal_pairs(group)

    import torch

    from . import _lib
    from .gpu.gpu_simulate import _buffer_addr

    # both stages read the block: a host block goes to the device once, here (alive until the calls return)
    on = torch.device("cuda", int(device))
    d, w = _on(on, data, run.cdt), None if weights is None else _on(on, weights, run.rdt)
    (d_ptr, d_dev), (w_ptr, w_dev) = _buffer_addr(d), _buffer_addr(w)
    _synchronize(on)
    tpol, ngroups, npairs, nd = 4 if polarized else 1, len(reds), len(pair1), int(pad) * run.nfreqs
    peak = np.zeros((nfeed, npairs), dtype=np.int32)
    x, power, total = (np.zeros((nfeed, npairs), dtype=np.float64) for _ in range(3))
    used = np.zeros((nfeed, npairs), dtype=np.int32)
    _lib.check(_lib.lib().fv_firstcal_pair_delays(
        int(device), int(precision), run.nfreqs, run.ntimes, run.nbls, tpol, npairs, _lib.ptr(pair1), _lib.ptr(pair2), _lib.ptr(a1),
        _lib.ptr(a2), d_ptr, d_dev, w_ptr, w_dev, int(pad), _lib.ptr(peak), _lib.ptr(x), _lib.ptr(power), _lib.ptr(total),
        _lib.ptr(used)))
    pair_delays = x / (nd * dnu)
    # A tau = dtau over the used pairs, per feed: +1 at a2[k] and a1[k'], -1 at a1[k] and a2[k']
    A = np.zeros((npairs, nant))
    for col, sign in ((a2[pair1], 1.0), (a1[pair2], 1.0), (a1[pair1], -1.0), (a2[pair2], -1.0)):
        np.add.at(A, (np.arange(npairs), col), sign)
    tau, in_pair = np.zeros((nfeed, nant)), np.zeros((nfeed, nant), dtype=bool)
    alike = nfeed == 2 and np.array_equal(used[0], used[1])  # (the usual case: one factorisation for both feeds)
    for feeds in ([[0, 1]] if alike else [[f] for f in range(nfeed)]):
        rows = used[feeds[0]] != 0
        if rows.any():
            tau[feeds] = np.linalg.lstsq(A[rows], pair_delays[feeds][:, rows].T, rcond=None)[0].T
            in_pair[feeds] = np.abs(A[rows]).sum(axis=0) > 0
    tau[~in_pair] = 0.0
    slopes = np.ascontiguousarray(2.0 * np.pi * tau * dnu)
    niter, change = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float64)
    chi2 = np.zeros((run.nfreqs, run.ntimes), dtype=np.float64)
    solved = np.zeros((nfeed, nant), dtype=np.int32)
    uvis = np.zeros((run.nfreqs, run.ntimes, tpol, ngroups), dtype=np.complex128)
    vis_solved = np.zeros(uvis.shape, dtype=np.int32)
    _lib.check(_lib.lib().fv_firstcal_offsets(
        int(device), int(precision), run.nfreqs, run.ntimes, run.nbls, tpol, nant, _lib.ptr(a1), _lib.ptr(a2), ngroups, _lib.ptr(group),
        _lib.ptr(slopes), d_ptr, d_dev, w_ptr, w_dev, _lib.ptr(c), _lib.ptr(uvis), int(max_iter), float(tol), _lib.ptr(niter),
        _lib.ptr(change), _lib.ptr(chi2), _lib.ptr(solved), _lib.ptr(vis_solved)))
    if ref_ant is not None:  # (feed 0's phase, both feeds alike)
        c = c * np.exp(-1j * np.angle(c[0, list(run.ants).index(ref_ant)]))
    gains = c[:, :, None] * np.exp(2j * np.pi * tau[:, :, None] * (nu - nu.mean()))  # (nfeed, nant, nfreqs)
    out_shape = run.vis_shape[:-1] + (ngroups,)
    out = _follow(data, gains=np.ascontiguousarray(gains.transpose(1, 0, 2)).reshape(lead + (run.nfreqs,)), vis=uvis.reshape(out_shape),
                  delays=np.ascontiguousarray(tau.T).reshape(lead), offsets=np.array(c.T, order="C").reshape(lead), chi2=chi2,
                  pair_delays=pair_delays.reshape((2, npairs) if polarized else (npairs,)),
                  pair_used=(used != 0).reshape((2, npairs) if polarized else (npairs,)),
                  solved=np.ascontiguousarray(((solved != 0) & in_pair).T).reshape(lead), vis_solved=(vis_solved != 0).reshape(out_shape))
    info = dict(delays=out["delays"], offsets=out["offsets"], pairs=[(baselines[i], baselines[j]) for i, j in zip(pair1, pair2)],
                pair_delays=out["pair_delays"], pair_used=out["pair_used"], niter=int(niter[0]),
                converged=bool(niter[0] > 0 and change[0] < tol), change=float(change[0]), chi2=out["chi2"], solved=out["solved"],
                vis_solved=out["vis_solved"], reds=reds, baselines=baselines)
    return out["gains"], out["vis"], info


def redundant_average(
    data,
    ants: dict,
    gains,
    *,
    reds: list = None,
    baselines: list = None,
    weights=None,
    polarized: bool = False,
    precision: int = 2,
    device: int = 0,
):
    """The calibrated, redundantly averaged data at any gains: the visibility step of ``redundant_gain_solve`` alone
    (``fv_redundant_vis_rows``).  Per (frequency, time, pol, group), over the group's used samples and with
    ``m = conj(g[a1]) g[a2]``:  ``den = sum w |m|^2``,  ``vis = sum w conj(m) d / den`` -- the least-squares group
    visibility for these gains, 0 where ``den == 0``.  ``data``, ``weights``, ``reds``, ``baselines`` as in
    ``redundant_gain_solve``; ``gains`` in any of ``simulate_vis_gain_chi2``'s four shapes, used in complex128.  Returns
    ``(vis, den)`` in ``redundant_gain_solve``'s layout of ``vis``, complex128 and float64, following ``data`` to its device."""
    run = _block_run(data, ants, polarized, precision, device)
    reds, baselines, group, a1, a2 = _block_inputs(run, ants, reds, baselines, data, weights)
    g = _gain_block(dataclasses.replace(run, cdt=np.complex128), gains)

    import torch

    from . import _lib

    # host arrays: the U-step on its own is a tool, not a loop's inner step
    d = np.ascontiguousarray(_host(data), dtype=run.cdt)
    w = None if weights is None else np.ascontiguousarray(_host(weights), dtype=run.rdt)
    _synchronize(torch.device("cuda", int(device)))
    tpol, ngroups, nrows = 4 if polarized else 1, len(reds), run.nfreqs * run.ntimes
    uvis = np.zeros((run.nfreqs, run.ntimes, tpol, ngroups), dtype=np.complex128)
    den = np.zeros(uvis.shape, dtype=np.float64)
    _lib.check(_lib.lib().fv_redundant_vis_rows(
        int(device), int(precision), nrows, run.nbls, tpol, len(run.ants), _lib.ptr(a1), _lib.ptr(a2), ngroups, _lib.ptr(group),
        _lib.ptr(g), _lib.ptr(d), _lib.ptr(w), _lib.ptr(uvis), _lib.ptr(den)))
    out_shape = run.vis_shape[:-1] + (ngroups,)
    out = _follow(data, vis=uvis.reshape(out_shape), den=den.reshape(out_shape))
    return out["vis"], out["den"]


_ABSCAL_MAX_GRID = 1 << 22


def _abscal_plane(ants: dict, reds):
    """The groups' baselines ``b_g = x[a2] - x[a1]`` of ``reds[g][0]`` and the plane they span: ``(b (ngroups, 3), Vt (ndim, 3),
    X = b Vt^T (ngroups, ndim))``.  ``ndim`` counts the singular values above 1e-9 of the largest (at least 1); 3 is a
    ValueError."""
    pos = {k: np.asarray(v, dtype=np.float64).reshape(-1)[:3] for k, v in ants.items()}
    b = np.array([pos[red[0][1]] - pos[red[0][0]] for red in reds], dtype=np.float64).reshape(len(reds), 3)
    cross = np.any(b != 0.0, axis=1)
    vt = np.eye(3)[:1]
    if cross.any():
        _, s, rows = np.linalg.svd(b[cross], full_matrices=False)
        ndim = max(1, int(np.sum(s > 1e-9 * s[0])))
        if ndim == 3:
            raise ValueError("the group baselines span three dimensions: redundant_abscal fits a slope on a line or in a plane "
                             "(rank 1 or 2); rank-3 arrays are not covered")
        vt = rows[:ndim]
    X = np.ascontiguousarray(b @ vt.T)
    X[~cross] = 0.0
    return b, vt, X


def _abscal_grid(X, b, max_slope, pad):
    """The search grid of ``redundant_abscal``: ``(n (2,), h (2,), max_slope)``; ``n[1] == 1`` for a line."""
    cross = np.any(b != 0.0, axis=1)
    ndim = X.shape[1]
    n, h = [1, 1], [1.0, 1.0]
    if not cross.any():
        return n, h, 0.0 if max_slope is None else float(max_slope)
    if max_slope is None:
        max_slope = np.pi / np.sqrt((b[cross] ** 2).sum(axis=1)).min()
    for i in range(ndim):
        extent = X[cross, i].max() - X[cross, i].min()
        if extent == 0.0:  # (a single baseline length)
            extent = np.abs(X[cross, i]).max()
        h[i] = 2.0 * np.pi / (pad * extent)
        n[i] = 2 * int(np.ceil(max_slope / h[i])) + 1
    if n[0] * n[1] > _ABSCAL_MAX_GRID:
        raise ValueError(f"the slope grid has {n[0]} x {n[1]} points, more than 2**22: pass a smaller max_slope (now {max_slope:.3e} "
                         "rad/m) or a smaller pad")
    return n, h, float(max_slope)


def redundant_abscal(
    vis,
    model,
    ants: dict,
    gains,
    *,
    reds: list = None,
    weights=None,
    per_time: bool = False,
    max_slope: float = None,
    pad: int = 4,
    refine: int = 6,
    polarized: bool = False,
    precision: int = 2,
    device: int = 0,
):
    """Absolute calibration on the device: fixes what redundant calibration leaves free -- per solve unit and feed the
    amplitude of the gains and a phase gradient across the array -- by fitting the group visibilities to a model of them
    (``fv_abscal_slopes``).  ``g_a -> g_a A exp(i Phi . (x_a - c))`` leaves the data model unchanged when ``U_g -> U_g eta
    exp(-i Phi . b_g)``, ``eta = A^-2``, ``b_g = x[a2] - x[a1]`` of ``reds[g][0] = (a1, a2)``; abscal minimises
    ``chi2(eta, Phi) = sum W |eta exp(-i Phi . b_g) U_g - M_g|^2`` over a unit's times and groups.  With ``c_g = sum_t W conj(U) M``,
    ``S(Phi) = sum_g c_g exp(i Phi . b_g)`` and ``N = sum W |U|^2`` the best ``eta`` is ``Re S / N`` and ``Phi`` maximises ``Re S``: a
    search over a grid of slopes (a non-uniform DFT from the group baselines, no unwrapping) and ``refine`` rounds of Newton.
    The overall phase cancels in every visibility and is not a parameter.  Returns ``(gains, info)``.

    * ``vis``: ``redundant_gain_solve``'s or ``redundant_average``'s group visibilities, ``(nfreqs, ntimes, ngroups)`` or
      ``(nfreqs, ntimes, 2, 2, ngroups)``, used in complex128.  ``model``: ``simulate_vis(..., baselines=[red[0] for red in reds])``
      in the same layout, used in the run's ``precision``.  ``weights``: per group in ``vis``' shape, float64, for instance
      ``redundant_average``'s ``den`` zeroed where ``vis_solved`` is False; None means ones.  Numpy arrays or tensors; a tensor
      on the run's device is read by pointer.  A sample is used when its weight is positive and its group is no
      auto-correlation's; a flagged datum is not read.  A negative or non-finite weight and a non-finite value at a used
      sample fail the call.
    * ``gains``: the gains to fix, in any of the gain solve's four shapes (None: ones).  Whether a unit is a frequency or a
      (frequency, time) follows their shape, by ``simulate_vis_gain_solve``'s shape rule and ``per_time``.
    * The slope lives in the span of the group baselines: the right singular vectors ``Vt`` of the ``(ngroups, 3)`` baseline
      matrix whose singular value exceeds 1e-9 of the largest, one for a line, two for a planar array; the device works in
      the in-plane coordinates ``X = B Vt^T``.  Three is a ValueError.
    * The grid, per dimension i: step ``h_i = 2 pi / (pad extent_i)``, ``extent_i = max X_i - min X_i``, and ``n_i = 2
      ceil(max_slope / h_i) + 1`` points centred on 0; ``max_slope`` defaults to ``pi / min |b_g|``.  On a lattice ``S`` is
      periodic in ``Phi``: aliased peaks give the same gains at every antenna.  The box is a square along the plane's axes: on
      a hexagonal lattice of spacing a it does not hold the corners of the reciprocal cell, at ``4 pi / (3 a)``, and
      ``max_slope=1.4 * np.pi / a`` does.  At most 2**22 points.
    * Polarized data fit the parallel hands, feed p reads ``[p, p]``, with one ``(eta, Phi)`` per feed.
    * Returns the gains times ``eta^-1/2 exp(i Phi . (x_a - mean x))`` per unit and feed, complex128, in ``gains``' shape.
      Antennas of units with ``used == False`` are unchanged.  The matching group visibilities are ``redundant_average`` at
      the returned gains.
    * ``info``, per unit and feed in the layout ``([2,] nfreqs[, ntimes])`` of the gains without their antenna axis: ``amp``
      (eta), ``slopes`` ``(..., 3)`` in ENU rad/m (the in-plane ``Phi`` mapped back through ``Vt``), ``used`` (False where ``N == 0``,
      fewer than ``ndim + 1`` groups are used or ``Re S <= 0``: eta = 1, Phi = 0), ``peak`` ``(..., 2)`` the grid point as signed
      steps, ``power`` (``Re S``), ``unorm`` (N), ``mnorm`` (``sum W |M|^2``); ``chi2`` ``(nfreqs, ntimes)`` at the returned
      parameters, summed over the feeds; ``grid``: a dict of ``n``, ``h`` and ``max_slope``; ``reds`` as used.

    Outputs follow ``vis`` to its device.  Not differentiable.  Not covered: one slope shared by both feeds and the
    cross-hand phase, a slope model across frequency (a delay slope), rank-3 arrays, Jones matrices, sharding over GPUs."""
    if int(pad) != pad or pad < 1:
        raise ValueError(f"pad must be a positive integer, got {pad!r}")
    if int(refine) != refine or not 0 <= refine <= 32:
        raise ValueError(f"refine must be an integer in 0 .. 32, got {refine!r}")
    if max_slope is not None and not (float(max_slope) > 0.0 and np.isfinite(float(max_slope))):
        raise ValueError(f"max_slope must be positive and finite (rad/m), got {max_slope!r}")
    run = _block_run(vis, ants, polarized, precision, device)
    reds, _, _ = _groups(ants, reds, None)
    ngroups = len(reds)
    if ngroups != run.nbls:
        raise ValueError(f"vis holds {run.nbls} groups, reds lists {ngroups}")
    _check_vis_block(run, vis, "vis")
    _check_vis_block(run, model, "model")
    if weights is not None:
        _check_weights(run, weights, "vis'")
        _run_device(run, (weights,), "weights")
    block, shape, own_time = _solve_start(run, gains, per_time)
    b, vt, X = _abscal_plane(run.ants, reds)
    n, h, max_slope = _abscal_grid(X, b, max_slope, int(pad))
    ndim = X.shape[1]

    import torch

    from . import _lib
    from .gpu.gpu_simulate import _buffer_addr

    def as_read(x, dtype):  # a tensor on the run's device by pointer, anything else as a host array
        if x is None:
            return None
        if _is_tensor(x) and x.device.type == "cuda":
            return _on(x.device, x, dtype)
        return np.ascontiguousarray(_host(x), dtype=dtype)

    u, m, w = as_read(vis, np.complex128), as_read(model, run.cdt), as_read(weights, np.float64)  # (alive until the call returns)
    (u_ptr, u_dev), (m_ptr, m_dev), (w_ptr, w_dev) = _buffer_addr(u), _buffer_addr(m), _buffer_addr(w)
    _synchronize(torch.device("cuda", int(device)))
    tpol, nfeed = (4, 2) if polarized else (1, 1)
    units = (run.nfreqs, run.ntimes if own_time else 1, nfeed)
    peak = np.zeros(units + (2,), dtype=np.int32)
    slopes = np.zeros(units + (2,), dtype=np.float64)
    amp, power, unorm, mnorm = (np.zeros(units, dtype=np.float64) for _ in range(4))
    used = np.zeros(units, dtype=np.int32)
    chi2 = np.zeros((run.nfreqs, run.ntimes), dtype=np.float64)
    _lib.check(_lib.lib().fv_abscal_slopes(
        int(device), int(precision), run.nfreqs, run.ntimes, tpol, ngroups, int(own_time), u_ptr, u_dev, m_ptr, m_dev, w_ptr, w_dev,
        _lib.ptr(X), ndim, n[0], n[1], float(h[0]), float(h[1]), int(refine), _lib.ptr(peak), _lib.ptr(slopes), _lib.ptr(amp),
        _lib.ptr(power), _lib.ptr(unorm), _lib.ptr(mnorm), _lib.ptr(used), _lib.ptr(chi2)))
    ok = used != 0
    enu = slopes[..., :ndim] @ vt  # (nfreqs, ntimes or 1, nfeed, 3)
    pos = np.array([run.ants[k].reshape(-1)[:3] for k in run.ants], dtype=np.float64)
    factor = np.exp(1j * (enu @ (pos - pos.mean(axis=0)).T)) / np.sqrt(amp)[..., None]  # (..., nfeed, nant)
    fixed = np.where(ok[..., None], block * factor, block)

    def unit(x):  # (nfreqs, ntimes or 1, nfeed, ...) in the gains' layout without the antenna axis
        tail = x.shape[3:]
        x = np.moveaxis(x, 2, 0)  # (nfeed, nfreqs, ntimes or 1, ...)
        lead = ((2,) if polarized else ()) + ((run.nfreqs, run.ntimes) if own_time else (run.nfreqs,))
        return np.ascontiguousarray(x).reshape(lead + tail)

    out = _follow(vis, gains=_solve_result(fixed, shape), amp=unit(amp), slopes=unit(enu), chi2=chi2, used=unit(ok), peak=unit(peak),
                  power=unit(power), unorm=unit(unorm), mnorm=unit(mnorm))
    info = dict(amp=out["amp"], slopes=out["slopes"], chi2=out["chi2"], used=out["used"], peak=out["peak"],
                grid=dict(n=tuple(n), h=tuple(h), max_slope=max_slope), power=out["power"], unorm=out["unorm"], mnorm=out["mnorm"],
                reds=reds)
    return out["gains"], info


def fix_redundant_degeneracies(gains, ants: dict, *, ref_gains=None, solved=None, tilt: str = "per_feed"):
    """Fix what redundant calibration leaves free.  Per solve unit and feed the data do not constrain four numbers: the
    amplitude of the gains, their overall phase, and a phase gradient across the array (``g_a -> g_a exp(i Phi . x_a)`` only
    moves every group's visibility by ``exp(-i Phi . b)``).  This brings them to those of ``ref_gains`` (None: ones) -- for
    instance a sky-based solve's.  On the host, in numpy: the work is nant-sized.

    * ``gains``, ``ref_gains``: ``(nant, ...)``, rows in ``ants``' order, any of the gain solve's shapes; ``solved``: a bool
      array of the same shape (``info["solved"]``), None for all.  Only solved antennas enter the fits and are changed.
    * Per column over the antennas: the gains are scaled by ``exp(mean log|ref| - mean log|g|)``; ``arg(g conj(ref))`` is
      fitted by ``psi + Phi . (x_a - mean x)`` over the antennas' positions by least squares (``lstsq``: the minimum-norm
      solution, so a flat array's ``Phi_z`` is 0), and the gains are multiplied by ``exp(-i (psi + Phi . (x_a - mean x)))``.
    * ``tilt="per_feed"`` fits every column on its own.  ``tilt="shared"`` takes axis 1 as the feed axis (polarized gains)
      and fits one ``Phi`` for both feeds, with a ``psi`` each: needed when cross-hands were used, which tie the feeds'
      gradients together.
    * The phase differences ``arg(g conj(ref))`` must lie inside ``(-pi, pi)``; there is no unwrapping.

    Returns the gains only, in ``gains``' shape, complex128.  The matching group visibilities are ``redundant_average`` at the
    returned gains."""
    if tilt not in ("per_feed", "shared"):
        raise ValueError(f'tilt must be "per_feed" or "shared", got {tilt!r}')
    g = np.array(_host(gains), dtype=np.complex128)
    nant = len(ants)
    if g.ndim < 1 or g.shape[0] != nant:
        raise ValueError(f"gains must have one row per antenna ({nant}), got shape {g.shape}")
    ref = np.ones_like(g) if ref_gains is None else np.asarray(_host(ref_gains), dtype=np.complex128)
    ok = np.ones(g.shape, dtype=bool) if solved is None else np.asarray(_host(solved), dtype=bool)
    if ref.shape != g.shape or ok.shape != g.shape:
        raise ValueError(f"ref_gains and solved must have gains' shape {g.shape}")
    if tilt == "shared" and (g.ndim < 2 or g.shape[1] != 2):
        raise ValueError(f'tilt="shared" needs polarized gains (nant, 2, ...), got shape {g.shape}')
    pos = np.array([np.asarray(ants[k], dtype=float) for k in ants]).reshape(nant, -1)
    nfeed = 2 if tilt == "shared" else 1
    # columns over the antennas: (nant, nfeed, units), the feeds of a unit fitted together when the tilt is shared
    cols = g.reshape(nant, nfeed, -1) if tilt == "shared" else g.reshape(nant, 1, -1)
    refs, oks = ref.reshape(cols.shape), ok.reshape(cols.shape)
    out = cols.copy()
    for u in range(cols.shape[2]):
        use = oks[:, :, u]
        if not use.any():
            continue
        centre = pos[use.any(axis=1)].mean(axis=0)
        x = pos - centre
        rows, rhs = [], []
        for f in range(nfeed):
            s = use[:, f]
            if not s.any():
                continue
            scale = np.exp(np.mean(np.log(np.abs(refs[s, f, u]))) - np.mean(np.log(np.abs(cols[s, f, u]))))
            out[s, f, u] = cols[s, f, u] * scale
            psi = np.zeros((int(s.sum()), nfeed))
            psi[:, f] = 1
            rows.append(np.hstack([psi, x[s]]))
            rhs.append(np.angle(cols[s, f, u] * np.conj(refs[s, f, u])))
        fit = np.linalg.lstsq(np.vstack(rows), np.concatenate(rhs), rcond=None)[0]
        for f in range(nfeed):
            s = use[:, f]
            out[s, f, u] *= np.exp(-1j * (fit[f] + x[s] @ fit[nfeed:]))
    out = out.reshape(g.shape)
    if _is_tensor(gains):
        import torch

        return torch.from_numpy(out).to(gains.device)
    return out
