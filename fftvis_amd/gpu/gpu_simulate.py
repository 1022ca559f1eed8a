"""GPU simulation engine: the filled-in ``GPUSimulationEngine`` of the reference
(stub at src/fftvis/gpu/gpu_simulate.py:20-91).

``simulate`` has the *CPU engine's* signature and return layout
(src/fftvis/cpu/cpu_simulate.py:537-569, 850-854) because that is what ``simulate_vis`` calls
(src/fftvis/wrapper.py:308-336); the stub's own narrower signature could not accept that call.
Host work here is one-time setup in numpy; every per-(time, frequency) computation happens in
libfftvis_hip (hand-written HIP kernels, no library FFT) behind the C ABI of include/fftvis_hip.h.  There is no CPU
fallback: without the library or a GPU the calls raise.
"""

from __future__ import annotations

import ctypes
import atexit
import contextlib
import logging
import types
import typing
import warnings

import numpy as np

from .. import _lib
from ..core import utils
from ..core.antenna_gridding import check_antpos_griddability
from ..core.beams import (airy_factors, checked_spline_order, describe_beam, feed_index, is_sampled_analytic,
                          table_tolerance)
from ..core.coords import SiderealRotation, eq_unit_vectors, julian_dates
from ..core.simulate import SimulationEngine, default_accuracy_dict

logger = logging.getLogger(__name__)


# Handles kept between ``simulate`` calls.  Creating and destroying a handle (streams, events, device
# buffers, per-geometry tables) costs ~15 ms, ten times the GPU work of a HERA-37 simulation -- and for a
# HERA-350 call ~85 ms of buffers, tables, launch lists and column plans that the next call on the same array
# would find ready; every ``fv_sim_set_*`` call fully replaces what it configures (re-setting what is already
# there keeps what was planned from it), so a handle whose creation parameters match can serve the next call.
# At most two idle handles, and only while this process holds less than FFTVIS_HIP_HANDLE_CACHE_BYTES of device
# memory (default: a quarter of the device's memory, at least 2 GiB; 0 = never keep one).
_IDLE_HANDLES: dict = {}
atexit.register(lambda: release_handles())


def _cache_limit(device: int = 0) -> int:
    import os

    env = os.environ.get("FFTVIS_HIP_HANDLE_CACHE_BYTES")
    if env is not None:
        return int(float(env))
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_mem_info(int(device), ctypes.byref(free), ctypes.byref(total)))
    return max(2 * 1024**3, total.value // 4)


def release_handles():
    """Destroy the idle handles and this thread's cached stand-alone NUFFT workspace (and free their
    device memory)."""
    while _IDLE_HANDLES:
        _IDLE_HANDLES.popitem()[1].close()
    if _lib._lib is not None:  # only if the library was ever loaded
        _lib._lib.fv_release_workspaces()


def _acquire_handle(device, precision, eps, upsample_factor, polarized):
    key = (int(device), int(precision), float(eps), str(upsample_factor), bool(polarized))
    h = _IDLE_HANDLES.pop(key, None)
    # the other idle handles of this device hold memory that wrapper.device_memory_budget counts as the run's:
    # released now (a matching handle's buffers are reused instead), as is the stand-alone NUFFT workspace on a miss
    for k in [k for k in _IDLE_HANDLES if k[0] == key[0]]:
        _IDLE_HANDLES.pop(k).close()
    if h is None and _lib._lib is not None:
        _lib._lib.fv_release_workspaces()
    return key, (h if h is not None else SimHandle(device, precision, eps, upsample_factor, polarized))


def _return_handle(key, h):
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(key[0], ctypes.byref(held)))
    limit = _cache_limit(key[0])
    if limit <= 0 or held.value > limit:
        h.close()
        return
    while len(_IDLE_HANDLES) >= 2:
        _IDLE_HANDLES.pop(next(iter(_IDLE_HANDLES))).close()
    _IDLE_HANDLES[key] = h


ADJOINT_PATHS = ("type3", "type2", "auto")


def _buffer_addr(a):
    """(address, on_device flag) of an adjoint buffer: a numpy array is a host buffer, a torch tensor a device buffer,
    None a null pointer (an output that is not wanted)."""
    if a is None:
        return None, 0
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data), 0
    return ctypes.c_void_p(a.data_ptr()), 1


class SimHandle:
    """RAII wrapper of one ``fv_sim`` handle (one GPU context)."""

    def __init__(self, device: int, precision: int, eps: float, upsample_factor: float,
                 polarized: bool):
        self._L = _lib.lib()
        _lib.require_gpu()
        self.precision = precision
        self.eps = float(eps)
        self.polarized = bool(polarized)
        self.rdt = np.float32 if precision == 1 else np.float64
        self.cdt = np.complex64 if precision == 1 else np.complex128
        self._h = ctypes.c_void_p()
        if upsample_factor in (None, "auto"):
            upsample_factor = 0.0  # the engine picks 2 or 1.25 per run (include/fftvis_hip.h, fv_sim_create)
        _lib.check(self._L.fv_sim_create(ctypes.byref(self._h), device, precision, float(eps),
                                         float(upsample_factor), int(polarized)))
        self.nbls = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.fv_sim_destroy(self._h)
            self._h = None

    __del__ = close

    # -- uploads ---------------------------------------------------------------------------
    def set_sources(self, eq, flux, polarized_sky: bool):
        eq = np.ascontiguousarray(eq, dtype=self.rdt)
        flux = np.ascontiguousarray(flux, dtype=self.cdt if polarized_sky else self.rdt)
        _lib.check(self._L.fv_sim_set_sources(self._h, eq.shape[1], flux.shape[1], _lib.ptr(eq),
                                              _lib.ptr(flux), int(polarized_sky), 0))

    def set_sources_device(self, nsrc, nfreq, eq_ptr, flux_ptr, polarized_sky: bool):
        """Device pointers (e.g. torch tensors filled by an RCCL broadcast)."""
        _lib.check(self._L.fv_sim_set_sources(self._h, nsrc, nfreq, _lib.ptr(eq_ptr),
                                              _lib.ptr(flux_ptr), int(polarized_sky), 1))

    def set_times(self, rot):
        rot = np.ascontiguousarray(rot, dtype=np.float64)
        _lib.check(self._L.fv_sim_set_times(self._h, rot.shape[0], _lib.ptr(rot)))

    def set_astrom(self, astrom):
        """(ntimes, 31) float64 eraASTROM contexts: per-source astrometry runs on the device (fv_sim_set_astrom)."""
        a = np.ascontiguousarray(astrom, dtype=np.float64)
        _lib.check(self._L.fv_sim_set_astrom(self._h, a.shape[0], _lib.ptr(a)))

    def set_topo(self, topo):
        topo = np.ascontiguousarray(topo, dtype=self.rdt)
        _lib.check(self._L.fv_sim_set_topo(self._h, topo.shape[0], topo.shape[2], _lib.ptr(topo), 0))

    def set_freqs(self, freqs):
        f = np.ascontiguousarray(freqs, dtype=np.float64)
        _lib.check(self._L.fv_sim_set_freqs(self._h, f.size, _lib.ptr(f)))

    def set_array(self, rotation_matrix, bls, is_coplanar: bool):
        R = np.ascontiguousarray(rotation_matrix, dtype=np.float64)
        b = np.ascontiguousarray(bls, dtype=np.float64)
        self.nbls = b.shape[1]
        _lib.check(self._L.fv_sim_set_array(self._h, _lib.ptr(R), self.nbls, _lib.ptr(b),
                                            int(is_coplanar)))

    def set_array_type1(self, basis_matrix, bls_int, n_modes: int):
        B = np.ascontiguousarray(basis_matrix, dtype=np.float64)
        b = np.ascontiguousarray(bls_int[:2], dtype=np.int32)
        self.nbls = b.shape[1]
        _lib.check(self._L.fv_sim_set_array_type1(self._h, _lib.ptr(B), self.nbls, _lib.ptr(b),
                                                  int(n_modes)))

    def set_beams(self, beam_list, freqs, order: int = 1, use_feed: str = "x"):
        _lib.check(self._L.fv_sim_set_nbeams(self._h, len(beam_list)))
        if beam_list and all(is_sampled_analytic(b) for b in beam_list):
            order = 3  # only third-party analytic beams: their tables (if any) are ours to lay out -- cubic
        for i, beam in enumerate(beam_list):
            d = describe_beam(beam, self.polarized, np.asarray(freqs, dtype=float), use_feed, order,
                              table_tolerance(self.eps))
            if d[0] == "airy":  # this package's AiryBeam, or a third-party object PROVEN to be that form x factors
                fac = airy_factors(d)
                _lib.check(self._L.fv_sim_set_beam_airy_scaled(self._h, i, d[1], _lib.ptr(fac), float(fac[8])))
            else:
                tab = d[1]
                _lib.check(self._L.fv_sim_set_beam_table(self._h, i, tab.shape[0], tab.shape[-2],
                                                         tab.shape[-1], float(d[2]), _lib.ptr(tab),
                                                         int(order)))

    def set_beam_pairs(self, pairs, pair_idx, pair_flip):
        bi = np.array([p[0] for p in pairs], dtype=np.int32)
        bj = np.array([p[1] for p in pairs], dtype=np.int32)
        off = np.zeros(len(pairs) + 1, dtype=np.int64)
        idx, flp = [], []
        for n, p in enumerate(pairs):
            ii = np.asarray(pair_idx[p], dtype=np.int32)
            off[n + 1] = off[n] + ii.size
            idx.append(ii)
            flp.append(np.asarray(pair_flip[p], dtype=np.int8))
        idx = np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0, np.int32))
        flp = np.ascontiguousarray(np.concatenate(flp) if flp else np.zeros(0, np.int8))
        if idx.size == 0:  # keep the pointers valid
            idx, flp = np.zeros(1, np.int32), np.zeros(1, np.int8)
        _lib.check(self._L.fv_sim_set_beam_pairs(self._h, len(pairs), _lib.ptr(bi), _lib.ptr(bj),
                                                 _lib.ptr(off), _lib.ptr(idx), _lib.ptr(flp)))

    def set_reference_compat(self, on: bool = True):
        """The reference's forms for flipped two-beam baselines / the eigenbeam (l, k) term, or the exact ones
        (fv_sim_set_reference_compat)."""
        _lib.check(self._L.fv_sim_set_reference_compat(self._h, int(bool(on))))

    def set_chunking(self, nchunks: int = 1, source_buffer: float = 1.0):
        """Source chunks per time step and the above-horizon buffer fraction (fv_sim_set_chunking)."""
        _lib.check(self._L.fv_sim_set_chunking(self._h, int(nchunks), float(source_buffer)))

    def set_basis(self, beam_coefs, ant1_idxs, ant2_idxs):
        c = np.ascontiguousarray(beam_coefs, dtype=self.cdt)
        a1 = np.ascontiguousarray(ant1_idxs, dtype=np.int32)
        a2 = np.ascontiguousarray(ant2_idxs, dtype=np.int32)
        _lib.check(self._L.fv_sim_set_basis(self._h, c.shape[0], c.shape[1], c.shape[2],
                                            _lib.ptr(c), _lib.ptr(a1), _lib.ptr(a2)))

    # -- execution ----------------------------------------------------------------------------
    def out_shape(self, nt, nf):
        return (nf, nt, 2, 2, self.nbls) if self.polarized else (nf, nt, self.nbls)

    def run(self, t0, t1, f0, f1, out=None, shared=False):
        """Times [t0,t1) x freqs [f0,f1) -> host array in the reference's final layout.

        ``out``: deliver into this array instead of a new one -- a block of a larger result, e.g.
        ``vis[fsl, tsl]`` (reference cpu_simulate.py:846-847): shape ``out_shape``, this engine's dtype, every axis
        but the first (channels) contiguous (``fv_sim_run_into``).  ``shared``: other processes fill the rest of the
        underlying array (a result in shared memory, one block per rank)."""
        shape = self.out_shape(t1 - t0, f1 - f0)
        if out is None:
            out = np.empty(shape, dtype=self.cdt)
            _lib.check(self._L.fv_sim_run(self._h, t0, t1, f0, f1, _lib.ptr(out), 0))
            return out
        if out.shape != shape or out.dtype != self.cdt or not out.flags.writeable:
            raise ValueError(f"out must be a writeable {np.dtype(self.cdt).name} array of shape {shape}, got {out.dtype} {out.shape}")
        inner = np.empty(shape[1:], dtype=self.cdt).strides
        if out.size and (out.strides[1:] != inner or out.strides[0] % out.itemsize or out.strides[0] < inner[0] * shape[1]):
            raise ValueError("out: only the first (channel) axis may be strided; the rest must be C-contiguous")
        if out.size:
            _lib.check(self._L.fv_sim_run_into(self._h, t0, t1, f0, f1, ctypes.c_void_p(out.ctypes.data),
                                               out.strides[0] // out.itemsize, int(bool(shared))))
        return out

    def _residual_pass(self, fn, t0, t1, f0, f1, data, weights, gvis, cal=()):
        """The body of the three objective calls, ``fn`` their entry point: ``cal`` is empty or (the gains or matrices, the
        array of their gradient or None).  Returns the (f1 - f0, t1 - t0) float64 rows."""
        x, grad = (_buffer_addr(c) for c in cal) if cal else ((), ())
        chi2 = np.empty((f1 - f0, t1 - t0), dtype=np.float64)
        _lib.check(fn(self._h, t0, t1, f0, f1, *_buffer_addr(data), *_buffer_addr(weights), *x, *_buffer_addr(gvis),
                      _lib.ptr(chi2), *grad))
        return chi2

    def _weight_pass(self, fn, t0, t1, f0, f1, parts, weights, cal=()):
        """The body of the three weighting calls, ``fn`` their entry point: ``cal`` is empty or (vis, the gains or matrices,
        their direction or None, the array of the H block or None).  Returns the (f1 - f0, t1 - t0) float64 rows."""
        ptrs = (ctypes.c_void_p * max(len(parts), 1))(*[p.data_ptr() for p in parts])
        vis, x, dx, grad = (_buffer_addr(c) for c in cal) if cal else ((), (), (), ())
        q = np.empty((f1 - f0, t1 - t0), dtype=np.float64)
        _lib.check(fn(self._h, t0, t1, f0, f1, len(parts), ptrs, *vis[:1], *_buffer_addr(weights), *x, *dx, _lib.ptr(q), *grad))
        return q

    def run_residual(self, t0, t1, f0, f1, data, weights, gvis):
        """The fit objective of times [t0,t1) x freqs [f0,f1) (``fv_sim_run_residual``): the forward run of the block goes
        into ``gvis`` and stays on the device, where ``gvis = 2 w (V - data)`` replaces it; returns the (f1 - f0, t1 - t0)
        float64 host array of ``sum w |V - data|^2`` per (frequency, time).  ``data`` and ``gvis``: C-contiguous blocks of
        ``out_shape(t1 - t0, f1 - f0)``, this engine's complex dtype; ``weights``: the same shape, this engine's real
        dtype, or None (every weight 1; 0 flags a sample).  numpy arrays are host buffers, torch tensors device buffers.
        ``gvis`` is what every ``run_*_adjoint`` takes as ``g``.  The call synchronises."""
        return self._residual_pass(self._L.fv_sim_run_residual, t0, t1, f0, f1, data, weights, gvis)

    def set_gain_pairs(self, nant, ant1_idxs, ant2_idxs):
        """The antenna pair of every baseline, as rows of the gains ``run_gain_residual`` takes (``fv_sim_set_gain_pairs``):
        after ``set_array`` / ``set_array_type1``, once per configured handle."""
        a1 = np.ascontiguousarray(ant1_idxs, dtype=np.int32)
        a2 = np.ascontiguousarray(ant2_idxs, dtype=np.int32)
        _lib.check(self._L.fv_sim_set_gain_pairs(self._h, int(nant), _lib.ptr(a1), _lib.ptr(a2)))

    def run_gain_residual(self, t0, t1, f0, f1, data, weights, gains, gvis, ggains=None):
        """``run_residual`` with per-antenna gains (``fv_sim_run_residual_gains``; ``set_gain_pairs`` first): the data model
        is ``V' = conj(g[a1]) g[a2] V``, ``gvis`` receives ``d chi2 / dV`` and the returned rows are
        ``sum w |V' - data|^2``.  ``gains``: C-contiguous (f1 - f0, t1 - t0, nfeed, nant), this engine's complex dtype;
        ``ggains``: the same shape, complex128, filled with the gradient with respect to the gains, or None (its kernel
        does not run).  numpy arrays are host buffers, torch tensors device buffers.  The call synchronises."""
        return self._residual_pass(self._L.fv_sim_run_residual_gains, t0, t1, f0, f1, data, weights, gvis, (gains, ggains))

    def run_jones_residual(self, t0, t1, f0, f1, data, weights, jones, gvis, gjones=None):
        """``run_gain_residual`` with one 2 x 2 complex matrix per antenna (``fv_sim_run_residual_jones``; ``set_gain_pairs``
        first, a polarized handle): antenna a's Jones matrix ``A_a[ax, feed]`` becomes ``A_a jones[a]``, on the output
        ``V'[x, y] = sum conj(J[a1][y', y]) J[a2][x', x] V[x', y']``; ``gvis`` receives ``d chi2 / dV`` and the returned rows
        are ``sum w |V' - data|^2``.  ``jones``: C-contiguous (f1 - f0, t1 - t0, 2, 2, nant), this engine's complex dtype,
        ``jones[f, t, i, j, a]`` with i the feed of the ideal antenna and j the measured one; ``gjones``: the same shape,
        complex128, filled with the gradient with respect to the matrices, or None (its kernel does not run).  numpy arrays
        are host buffers, torch tensors device buffers.  The call synchronises."""
        return self._residual_pass(self._L.fv_sim_run_residual_jones, t0, t1, f0, f1, data, weights, gvis, (jones, gjones))

    def weight_block(self, t0, t1, f0, f1, parts, weights):
        """The weighting step of a Gauss-Newton product for times [t0,t1) x freqs [f0,f1) (``fv_sim_weight_block``):
        ``parts`` -- one to four device tensors, each a C-contiguous block of ``out_shape(t1 - t0, f1 - f0)`` of this
        engine's complex dtype that a forward or tangent pass of this handle filled -- are summed in order, and
        ``parts[0] = 2 w (sum)`` replaces the first; returns the (f1 - f0, t1 - t0) float64 host array of ``sum w |sum|^2``
        per (frequency, time).  ``weights`` as for ``run_residual``.  ``parts[0]`` is then what every ``run_*_adjoint``
        takes as ``g``.  The call synchronises."""
        return self._weight_pass(self._L.fv_sim_weight_block, t0, t1, f0, f1, parts, weights)

    def gain_weight_block(self, t0, t1, f0, f1, parts, vis, weights, gains, d_gains=None, hgains=None):
        """``weight_block`` with per-antenna gains and a gain direction (``fv_sim_gain_weight_block``; ``set_gain_pairs``
        first): with ``m = conj(g[a1]) g[a2]``, ``dm`` its tangent along ``d_gains`` and U the sum of ``parts`` -- none to
        four device tensors; none is the gains-only direction --, ``U' = m U + dm V`` is the tangent of the data model,
        ``G = conj(m) 2 w U'`` replaces ``parts[0]`` (``vis`` when there are no parts) and the returned rows are
        ``sum w |U'|^2``.  ``vis``: the device tensor a forward run of this handle filled with V, needed with ``d_gains``,
        with ``hgains`` and without parts, else None.  ``gains``, ``d_gains`` (or None): C-contiguous (f1 - f0, t1 - t0,
        nfeed, nant), this engine's complex dtype; ``hgains``: the same shape, complex128, filled with the gain block of
        H p, or None (its kernel does not run).  numpy arrays are host buffers, torch tensors device buffers.  The
        stored G is what every ``run_*_adjoint`` takes as ``g``.  The call synchronises."""
        return self._weight_pass(self._L.fv_sim_gain_weight_block, t0, t1, f0, f1, parts, weights, (vis, gains, d_gains, hgains))

    def jones_weight_block(self, t0, t1, f0, f1, parts, vis, weights, jones, d_jones=None, hjones=None):
        """``gain_weight_block`` with one 2 x 2 complex matrix per antenna and a direction of such matrices
        (``fv_sim_jones_weight_block``; ``set_gain_pairs`` first, a polarized handle): with ``S(X; A, B)[x, y] = sum
        conj(A[y', y]) B[x', x] X[x', y']`` the data model's product and U the sum of ``parts`` -- none to four device
        tensors; none is the matrices-only direction --, ``U' = S(U; J[a1], J[a2]) + S(V; dJ[a1], J[a2]) + S(V; J[a1],
        dJ[a2])`` is the tangent of the data model, the transposed product applied to ``2 w U'`` replaces ``parts[0]``
        (``vis`` when there are no parts) and the returned rows are ``sum w |U'|^2``.  ``vis``: the device tensor a forward
        run of this handle filled with V, needed with ``d_jones``, with ``hjones`` and without parts, else None.  ``jones``,
        ``d_jones`` (or None): C-contiguous (f1 - f0, t1 - t0, 2, 2, nant), this engine's complex dtype; ``hjones``: the same
        shape, complex128, filled with the matrices' block of H p, or None (its kernel does not run).  numpy arrays are host
        buffers, torch tensors device buffers.  The stored G is what every ``run_*_adjoint`` takes as ``g``.  The call
        synchronises."""
        return self._weight_pass(self._L.fv_sim_jones_weight_block, t0, t1, f0, f1, parts, weights, (vis, jones, d_jones, hjones))

    def run_adjoint(self, t0, t1, f0, f1, g, gflux, accumulate: bool):
        """``gflux += A^T g`` for times [t0,t1) x freqs [f0,f1) (``fv_sim_run_adjoint``).  ``g``: C-contiguous block of
        ``out_shape(t1 - t0, f1 - f0)``, this engine's complex dtype; ``gflux``: C-contiguous (nsrc, nfreq) real or
        (nsrc, nfreq, 2, 2) complex.  numpy arrays are host buffers, torch tensors device buffers (ready when the call
        is made: the library's streams do not follow torch's).  The call synchronises."""
        gp, g_dev = _buffer_addr(g)
        fp, f_dev = _buffer_addr(gflux)
        _lib.check(self._L.fv_sim_run_adjoint(self._h, t0, t1, f0, f1, gp, g_dev, fp, f_dev, int(bool(accumulate))))

    def set_adjoint_path(self, path: str = "type3"):
        """The transform ``run_adjoint`` uses on a lattice handle (``fv_sim_set_adjoint_path``): ``"type3"`` the type-3
        transform with the roles swapped, ``"type2"`` the transpose of the type-1 slice."""
        _lib.check(self._L.fv_sim_set_adjoint_path(self._h, {"type3": 0, "type2": 1}[path]))

    def last_adjoint_path(self) -> int:
        """What this handle's last ``run_adjoint`` took (``fv_sim_last_adjoint_path``): 0 none yet, 2 or 3."""
        return int(self._L.fv_sim_last_adjoint_path(self._h))

    def run_basis_adjoint(self, t0, t1, f0, f1, g, gflux, gcoefs, accumulate: bool):
        """Basis beams (``set_basis``): ``gflux += A^T g`` and ``gcoefs +=`` the coefficient gradient for times [t0,t1) x
        freqs [f0,f1) (``fv_sim_run_basis_adjoint``).  ``g`` and ``gflux`` as for ``run_adjoint``; ``gcoefs``: C-contiguous
        (nant, nbasis, nfreq) of this engine's complex dtype.  Either output may be None (its pass does not run)."""
        gp, g_dev = _buffer_addr(g)
        fp, f_dev = _buffer_addr(gflux)
        cp, c_dev = _buffer_addr(gcoefs)
        _lib.check(self._L.fv_sim_run_basis_adjoint(self._h, t0, t1, f0, f1, gp, g_dev, fp, f_dev, cp, c_dev,
                                                    int(bool(accumulate))))

    def run_position_adjoint(self, t0, t1, f0, f1, g, gbls, accumulate: bool):
        """``gbls +=`` the gradient with respect to the baseline vectors for times [t0,t1) x freqs [f0,f1)
        (``fv_sim_run_position_adjoint``).  ``g`` as for ``run_adjoint``; ``gbls``: C-contiguous (nbls, 3) float64 at
        either precision, per metre, in the frame the antenna positions were given in."""
        gp, g_dev = _buffer_addr(g)
        bp, b_dev = _buffer_addr(gbls)
        _lib.check(self._L.fv_sim_run_position_adjoint(self._h, t0, t1, f0, f1, gp, g_dev, bp, b_dev, int(bool(accumulate))))

    def run_basis_position_adjoint(self, t0, t1, f0, f1, g, gbls, accumulate: bool):
        """Basis beams (``set_basis``): ``gbls +=`` the gradient with respect to the baseline vectors for times [t0,t1) x
        freqs [f0,f1) (``fv_sim_run_basis_position_adjoint``).  ``g`` and ``gbls`` as for ``run_position_adjoint``."""
        gp, g_dev = _buffer_addr(g)
        bp, b_dev = _buffer_addr(gbls)
        _lib.check(self._L.fv_sim_run_basis_position_adjoint(self._h, t0, t1, f0, f1, gp, g_dev, bp, b_dev,
                                                             int(bool(accumulate))))

    def run_source_adjoint(self, t0, t1, f0, f1, g, gtopo, accumulate: bool):
        """``gtopo +=`` the tangential gradient with respect to the sources' ENU unit vectors for times [t0,t1) x freqs
        [f0,f1) (``fv_sim_run_source_adjoint``).  ``g`` as for ``run_adjoint``; ``gtopo``: C-contiguous (t1 - t0, nsrc, 3)
        float64 at either precision.  The handle's fluxes are the forward's."""
        gp, g_dev = _buffer_addr(g)
        tp, t_dev = _buffer_addr(gtopo)
        _lib.check(self._L.fv_sim_run_source_adjoint(self._h, t0, t1, f0, f1, gp, g_dev, tp, t_dev, int(bool(accumulate))))

    def run_tangent(self, t0, t1, f0, f1, dbls, dtopo, out):
        """``out =`` the tangent of the visibilities along ``dbls`` and / or ``dtopo`` for times [t0,t1) x freqs [f0,f1)
        (``fv_sim_run_tangent``).  ``dbls``: C-contiguous (nbls, 3) float64, metres, in the frame the antenna positions
        were given in; ``dtopo``: C-contiguous (t1 - t0, nsrc, 3) float64, ENU; either may be None, not both.  ``out``:
        C-contiguous block of ``out_shape(t1 - t0, f1 - f0)``, this engine's complex dtype, overwritten.  numpy arrays are
        host buffers, torch tensors device buffers.  The call synchronises."""
        bp, b_dev = _buffer_addr(dbls)
        tp, t_dev = _buffer_addr(dtopo)
        op, o_dev = _buffer_addr(out)
        _lib.check(self._L.fv_sim_run_tangent(self._h, t0, t1, f0, f1, bp, b_dev, tp, t_dev, op, o_dev))

    def run_basis_position_tangent(self, t0, t1, f0, f1, dbls, out):
        """Basis beams (``set_basis``): ``out =`` the tangent of the visibilities along ``dbls`` for times [t0,t1) x freqs
        [f0,f1) (``fv_sim_run_basis_position_tangent``).  ``dbls`` and ``out`` as for ``run_tangent``."""
        bp, b_dev = _buffer_addr(dbls)
        op, o_dev = _buffer_addr(out)
        _lib.check(self._L.fv_sim_run_basis_position_tangent(self._h, t0, t1, f0, f1, bp, b_dev, op, o_dev))

    def run_basis_source_adjoint(self, t0, t1, f0, f1, g, gtopo, accumulate: bool):
        """Basis beams (``set_basis``): ``gtopo +=`` the tangential gradient with respect to the sources' ENU unit vectors
        for times [t0,t1) x freqs [f0,f1) (``fv_sim_run_basis_source_adjoint``).  ``g`` and ``gtopo`` as for
        ``run_source_adjoint``."""
        gp, g_dev = _buffer_addr(g)
        tp, t_dev = _buffer_addr(gtopo)
        _lib.check(self._L.fv_sim_run_basis_source_adjoint(self._h, t0, t1, f0, f1, gp, g_dev, tp, t_dev,
                                                           int(bool(accumulate))))

    def run_sky_adjoint(self, t0, t1, f0, f1, g, gflux, gtopo, accumulate: bool, basis: bool = False):
        """``gflux += A^T g`` and ``gtopo +=`` the sources' tangential gradient from one pass for times [t0,t1) x freqs
        [f0,f1) (``fv_sim_run_sky_adjoint``; ``basis``: ``fv_sim_run_basis_sky_adjoint``, a handle with ``set_basis``).
        ``g`` and ``gflux`` as for ``run_adjoint``, ``gtopo`` as for ``run_source_adjoint``; ``accumulate`` applies to
        both outputs."""
        gp, g_dev = _buffer_addr(g)
        fp, f_dev = _buffer_addr(gflux)
        tp, t_dev = _buffer_addr(gtopo)
        fn = self._L.fv_sim_run_basis_sky_adjoint if basis else self._L.fv_sim_run_sky_adjoint
        _lib.check(fn(self._h, t0, t1, f0, f1, gp, g_dev, fp, f_dev, tp, t_dev, int(bool(accumulate))))

    def run_basis_source_tangent(self, t0, t1, f0, f1, dtopo, out):
        """Basis beams (``set_basis``): ``out =`` the tangent of the visibilities along ``dtopo`` for times [t0,t1) x freqs
        [f0,f1) (``fv_sim_run_basis_source_tangent``).  ``dtopo`` and ``out`` as for ``run_tangent``."""
        tp, t_dev = _buffer_addr(dtopo)
        op, o_dev = _buffer_addr(out)
        _lib.check(self._L.fv_sim_run_basis_source_tangent(self._h, t0, t1, f0, f1, tp, t_dev, op, o_dev))

    def run_basis_tangent(self, t0, t1, f0, f1, dcoefs, out):
        """Basis beams (``set_basis``): ``out[q] =`` the tangent of the visibilities along direction ``dcoefs[q]`` of the
        coefficients for times [t0,t1) x freqs [f0,f1) (``fv_sim_run_basis_tangent``).  ``dcoefs``: C-contiguous
        (ndir, nant, nbasis, nfreq) of this engine's complex dtype; ``out``: C-contiguous
        (ndir,) + ``out_shape(t1 - t0, f1 - f0)``, the same dtype, overwritten.  numpy arrays are host buffers, torch
        tensors device buffers.  The directions share every transform.  The call synchronises."""
        dp, d_dev = _buffer_addr(dcoefs)
        op, o_dev = _buffer_addr(out)
        _lib.check(self._L.fv_sim_run_basis_tangent(self._h, t0, t1, f0, f1, dp, d_dev, int(dcoefs.shape[0]), op, o_dev))

    def run_device(self, t0, t1, f0, f1, out_ptr):
        """Enqueue only; ``out_ptr`` is a device buffer of out_shape() complex elements."""
        _lib.check(self._L.fv_sim_run(self._h, t0, t1, f0, f1, _lib.ptr(out_ptr), 1))

    def sync(self):
        _lib.check(self._L.fv_sim_sync(self._h))

    def stats(self):
        v = np.zeros(20)
        _lib.check(self._L.fv_sim_stats(self._h, _lib.ptr(v), 20))
        # ("n2z" is historical: active cells na_x * 65536 + na_y; the third dimension's sizes are n2_3 / na_3)
        keys = ["spread_launches", "spread_cells", "source_visits", "fft_cells", "interp_items",
                "sources_above_horizon", "n2x", "n2y", "n2z", "w", "upsample_used", "max_above_horizon", "fft_flops",
                "n2_3", "na_3", "height_terms", "lanes", "lane_mode", "height_terms_light_from", "height_terms_lighter_from"]
        return dict(zip(keys, v))

    def reset_stats(self):
        _lib.check(self._L.fv_sim_reset_stats(self._h))

    def enable_timing(self, on=True):
        _lib.check(self._L.fv_sim_enable_timing(self._h, int(on)))

    def timing(self):
        v = np.zeros(6)
        _lib.check(self._L.fv_sim_timing(self._h, _lib.ptr(v), 6))
        return dict(zip(["spread", "fft", "interp", "strengths", "prep", "spread_launches_timed"], v))


def register_with_reference() -> bool:
    """Make ``isinstance(engine, fftvis.core.simulate.SimulationEngine)`` hold where the reference is
    installed (virtual-subclass registration on its ABC, core/simulate.py:22).  Lazy: importing this module
    registers only if ``fftvis.core.simulate`` is ALREADY imported (importing the reference pulls in finufft,
    matvis, astropy and pyuvdata -- seconds, for an ``ABC.register``), the first ``GPUSimulationEngine()`` tries
    again if the caller has imported ``fftvis`` since, and the stub module of INTEGRATION.md, route A, calls this
    function itself (which does import ``fftvis.core.simulate``).  Only a missing reference is swallowed: any other
    error of that import is the caller's to see."""
    global _REGISTERED
    import sys

    mod = sys.modules.get("fftvis.core.simulate")
    if mod is None:
        import importlib

        try:
            mod = importlib.import_module("fftvis.core.simulate")
        except ImportError:  # the reference (or one of its dependencies) is not installed
            return False
    mod.SimulationEngine.register(GPUSimulationEngine)
    _REGISTERED = True
    return True


_REGISTERED = False


def prepare_array(ants: dict, baselines, flat_array_tol: float, real_dtype):
    """Plane-fit rotation, rotated baselines in seconds, coplanarity flag
    (reference cpu_simulate.py:628-659)."""
    antkey_to_idx = {a: i for i, a in enumerate(ants)}
    antvecs = np.array([ants[a] for a in ants], dtype=real_dtype)
    R = np.ascontiguousarray(utils.get_plane_to_xy_rotation_matrix(antvecs).T)
    rot = R @ antvecs.T
    i0 = np.array([antkey_to_idx[b[0]] for b in baselines], dtype=int)
    i1 = np.array([antkey_to_idx[b[1]] for b in baselines], dtype=int)
    bls = (rot[:, i1] - rot[:, i0]).reshape(3, len(baselines)).astype(float)
    is_coplanar = bool(np.all(np.abs(bls[2]) <= flat_array_tol))
    bls = (bls / utils.speed_of_light).astype(real_dtype)
    return R.astype(real_dtype), bls, is_coplanar


class GPUSimulationEngine(SimulationEngine):
    """MI355X implementation of the simulation engine."""

    def __init__(self, device: int = 0):
        import sys

        if not _REGISTERED and "fftvis" in sys.modules:  # the caller uses the reference: be an instance of ITS ABC
            register_with_reference()
        self.device = device

    def simulate(
        self,
        ants: dict,
        freqs: np.ndarray,
        fluxes: np.ndarray,
        beam_list: list,
        ra: np.ndarray,
        dec: np.ndarray,
        times,
        telescope_loc,
        baselines: list = None,
        beam_idx: np.ndarray = None,
        precision: int = 2,
        polarized: bool = False,
        eps: float = None,
        upsample_factor=2,
        beam_spline_opts: dict = None,
        flat_array_tol: float = 1e-6,
        interpolation_function: str = "az_za_map_coordinates",
        nprocesses: int | None = 1,
        nthreads: int | None = None,
        coord_method: str = "CoordinateRotationERFA",
        coord_method_params: dict | None = None,
        force_use_ray: bool = False,
        force_use_type3: bool = False,
        trace_mem: bool = False,
        enable_memory_monitor: bool = False,
        nchunks: int = 1,
        source_buffer=1.0,
        beam_coefs: np.ndarray = None,
        coord_mgr=None,
        time_idx: slice = slice(None),
        freq_idx: slice = slice(None),
        use_feed: str = "x",
        catalog_device=None,
        reference_compat: bool = True,
        astrom: np.ndarray = None,
        device_astrometry: bool = False,
        out: np.ndarray = None,
        out_shared: bool = False,
        adjoint_of: tuple = None,
        adjoint_path: str = "type3",
        adjoint_wrt: str = "fluxes",
        tangent_of: tuple = None,
        basis_tangent_of: tuple = None,
        basis_source_of: tuple = None,
        sky_of: tuple = None,
        objective_of: tuple = None,
        gauss_newton_of: tuple = None,
        forward_to=None,
    ) -> np.ndarray:
        """Simulate visibilities on the GPU.

        Same arguments and return value as ``CPUSimulationEngine.simulate``
        (reference cpu_simulate.py:537-854).  Differences, all documented in DESIGN.md:

        * like the reference, a flat array whose antennas sit on a lattice takes the type-1 path
          unless ``force_use_type3`` (cpu_simulate.py:634-637); eigenbeam runs always use type 3
          here;
        * ``coord_method``: as in the reference (cpu_simulate.py:686-709) the engine builds matvis' coordinate
          manager ``CoordinateRotation._methods[coord_method]`` itself when the caller passes none (matvis and
          astropy are imported lazily, here only; without them the call raises ValueError) and uses its per-time
          topocentric vectors (``rotate(ti)`` -> ``all_coords_topo``) verbatim, streamed to the device one time
          block at a time; a caller-built manager can be handed over as ``coord_mgr`` (extra).  The
          mean-sidereal rotation of ``core/coords.py`` (no precession / nutation / aberration: ~0.35 deg off
          ICRS positions at 2025 epochs) runs only when asked for by name, ``coord_method="SiderealRotation"``;
        * ``astrom`` / ``device_astrometry`` (extra; SURVEY section 8 f3 -- the coordinate manager on the device):
          ``astrom`` = (ntimes, 31) float64, one ERFA ``eraASTROM`` context per time (``erfa.apco13`` / astropy's
          ``erfa_astrom.apco`` fill it in microseconds); the device applies it to every source -- light deflection,
          aberration, bias-precession-nutation, Earth rotation, polar motion, diurnal aberration, horizon frame,
          refraction (``fv_sim_set_astrom``) -- so no (ntimes, 3, nsrc) vectors are computed or streamed on the host.
          ``device_astrometry=True`` builds the contexts here with astropy (the context astropy's own ICRS -> AltAz
          uses; raises ValueError without astropy) instead of building the matvis manager.  Default off: the
          reference's manager stays the default route.  Unpinned against ERFA in this pipeline;
        * ``nchunks`` splits the source axis exactly like the reference's chunk loop
          (cpu_simulate.py:939,1024,1069): every time step processes the catalog in ``nchunks`` pieces
          whose visibilities accumulate on the device; ``source_buffer`` sizes the above-horizon
          arrays of a piece and a piece that overflows them raises, as matvis does.  On top of that the
          engine walks the time axis in blocks when the output block would not fit in free device
          memory;
        * ``nprocesses/nthreads/force_use_ray/trace_mem/enable_memory_monitor`` are CPU scheduling /
          tracing knobs with no meaning on one GPU (``n_threads`` "not used in GPU implementation",
          reference gpu/nufft.py:38): accepted, unused;
        * ``beam_coefs`` (eigenbeams): like the reference, the (l, k) term reuses V_kl transposed
          (exact for real-valued basis beams, reference cpu_simulate.py:464-468);
        * ``reference_compat`` (extra, default True = the reference's arithmetic): False switches the two places
          where the reference departs from the exact symmetry of the visibilities to the
          exact forms -- flipped baselines of a two-beam polarized pair become V_ij(-b)^H (conjugated AND feed
          block transposed; the reference only conjugates, cpu_simulate.py:298), and the eigenbeam (l, k) term
          becomes conj(V_kl(-b))^T (one more gather at -b; exact for complex basis beams too);
        * ``beam_spline_opts``: orders 0 .. 5 as scipy.ndimage.map_coordinates takes them (1 = bilinear, also when
          None; 3 = cubic B-spline; ``kx/ky`` of ``az_za_simple`` are read the same way -- both interpolation
          functions of the reference are regular-grid splines of that order and map onto the same device
          interpolant); other orders raise ValueError;
        * ``use_feed`` (extra; the reference's wrapper applies it before the engine,
          wrapper.py:278-279): the feed whose power pattern an unpolarized run takes from an E-field beam;
        * ``upsample_factor``: 2 (default, as the reference) or 1.25 are used as given; ``None`` /
          ``"auto"`` (extra) lets the engine pick per run -- 1.25 when eps >= 1e-8 (fp32: 1e-4) and
          the fine grid is large (HERA-350 class arrays: ~2x faster), else 2;
        * ``time_idx`` / ``freq_idx`` (extra) restrict the run to a block, which is how ranks
          shard a simulation across GPUs; ``catalog_device`` (extra; ``parallel.DeviceCatalog``) is a
          catalog already resident on this GPU -- e.g. received by an RCCL broadcast -- used instead
          of ``ra / dec / fluxes`` (which may then be None);
        * ``out`` (extra): deliver the block into this array -- typically a view ``vis[freq_idx, time_idx]`` of the
          whole result, the reference's ``vis[tc][..., fc] = future`` (cpu_simulate.py:846-847) without the copy --
          of the block's shape and dtype, only its channel axis strided; it is pinned in place and filled while the
          run computes.  ``out_shared`` (extra): the underlying array is shared memory that other ranks fill too
          (``parallel.simulate_vis_sharded``).
        * The eight mode keywords below -- ``adjoint_of``, ``tangent_of``, ``basis_tangent_of``, ``basis_source_of``,
          ``sky_of``, ``objective_of``, ``gauss_newton_of``, ``forward_to`` -- each replace the forward run by another pass of
          the engine these arguments configure, and exclude each other: two of them in one call are a ValueError whose
          message is the later one's in that order, raised before anything else is looked at.
        * ``adjoint_of`` (extra; what ``simulate_vis_adjoint`` passes): a pair ``(g, gflux)`` -- instead of simulating,
          the engine configured by these arguments adds the adjoint of its map from ``fluxes`` (which then only give
          the catalog's shape) to visibilities, applied to ``g`` (the result's shape, this precision's complex dtype),
          into ``gflux`` (``SimHandle.run_adjoint``) and returns ``gflux``.  With ``beam_coefs`` (what
          ``simulate_vis_basis_adjoint`` passes) a triple ``(g, gflux, gcoefs)``, either output None when not wanted:
          ``SimHandle.run_basis_adjoint`` adds both gradients (``fluxes`` are then the forward's) and the call returns
          ``(gflux, gcoefs)``.  A fourth entry ``gbls``, (nbls, 3) float64 or None, also asks for the gradient with respect
          to the baseline vectors (``SimHandle.run_basis_position_adjoint``, per time block after the other two) and the
          call returns ``(gflux, gcoefs, gbls)``; every pass runs only when its output is given.
        * ``adjoint_wrt`` (extra; with ``adjoint_of``, no basis beams): ``"fluxes"`` (default) as above; ``"positions"`` (what
          ``simulate_vis_position_adjoint`` passes): ``adjoint_of`` is ``(g, gbls)`` and the engine adds the gradient with
          respect to the baseline vectors into ``gbls``, (nbls, 3) float64 (``SimHandle.run_position_adjoint``), and
          returns it.  The pass runs the type-3 transform only: ValueError on the lattice path (pass
          ``force_use_type3=True``) and with ``beam_coefs``.  ``"sources"`` (what ``simulate_vis_source_adjoint`` passes):
          ``adjoint_of`` is ``(g, gtopo)`` and the engine fills ``gtopo``, (ntimes, nsrc, 3) float64, with the tangential
          gradient with respect to the sources' ENU unit vectors, row t from time step t
          (``SimHandle.run_source_adjoint``), and returns it; the same restrictions.
        * ``adjoint_path`` (extra; with ``adjoint_of``, no basis beams): ``"type3"`` (default) the type-3 transform with
          the roles swapped; ``"type2"`` the transpose of the lattice path's type-1 slice -- ValueError when these
          arguments do not take the lattice path (not griddable, not flat, ``force_use_type3``, basis beams);
          ``"auto"`` type 2 exactly where the forward takes type 1, type 3 elsewhere.
        * ``tangent_of`` (extra; what ``simulate_vis_jvp`` passes): a triple ``(dbls, dtopo, dv)`` -- instead of simulating,
          the engine fills ``dv`` (the result's shape, this precision's complex dtype) with the tangent of its
          visibilities along a change ``dbls`` (nbls, 3) of the baseline vectors and / or ``dtopo`` (ntimes, nsrc, 3) of
          the sources' ENU unit vectors, either None (``SimHandle.run_tangent``), and returns it.  Time blocks take
          consecutive rows of ``dtopo``.  The pass runs the type-3 transform only: ValueError on the lattice path (pass
          ``force_use_type3=True``).  With ``beam_coefs`` (what ``simulate_vis_basis_jvp`` passes for a position tangent)
          only ``dbls`` is served (``SimHandle.run_basis_position_tangent``); a ``dtopo`` there is a ValueError.
        * ``basis_tangent_of`` (extra; what ``simulate_vis_basis_jvp`` passes; needs ``beam_coefs``): a pair ``(dcoefs, dv)``
          -- instead of simulating, the engine fills ``dv``, (ndir,) + the result's shape, this precision's complex dtype,
          with the tangents of its visibilities along the ``ndir`` directions ``dcoefs`` (ndir, nant, nbasis, nfreqs) of the
          coefficients (``SimHandle.run_basis_tangent``: one forward run, whatever ``ndir``) and returns it.
        * ``basis_source_of`` (extra; what ``simulate_vis_basis_source_adjoint`` / ``_jvp`` pass; needs ``beam_coefs``): the
          source-direction passes through basis beams.  ``("adjoint", g, gtopo)``: the engine fills ``gtopo``,
          (ntimes, nsrc, 3) float64, with the tangential gradient with respect to the sources' ENU unit vectors, row t
          from time step t (``SimHandle.run_basis_source_adjoint``), and returns it.  ``("tangent", dtopo, dv)``: it fills
          ``dv`` (the result's shape) with the tangent along ``dtopo`` (ntimes, nsrc, 3)
          (``SimHandle.run_basis_source_tangent``) and returns it.  Time blocks take consecutive rows.
        * ``sky_of`` (extra; what ``simulate_vis_sky_adjoint`` / ``simulate_vis_basis_sky_adjoint`` pass): a triple
          ``(g, gflux, gtopo)`` -- the joint sky adjoint, with or without ``beam_coefs``: one pass per time block
          (``SimHandle.run_sky_adjoint``) adds the flux gradient of ``adjoint_of`` into ``gflux`` and fills the block's rows
          of ``gtopo`` as ``adjoint_wrt="sources"`` / ``basis_source_of`` do; returns ``(gflux, gtopo)``.  The pass runs the
          type-3 transform only: ValueError on the lattice path (pass ``force_use_type3=True``).
        * ``objective_of`` (extra; what ``simulate_vis_chi2`` passes): a triple ``(data, weights, outputs)`` -- the fit
          objective chi2 = sum w |V - data|^2 and its gradients from one handle and one set-up, V never leaving the
          device.  ``data`` (the result's shape, this precision's complex dtype) and ``weights`` (the same shape, real, or
          None) are numpy arrays or tensors on this device.  ``outputs`` is a dict of zeroed buffers, each optional:
          ``"gflux"``, ``"gcoefs"``, ``"gbls"`` and ``"gtopo"`` as the modes above take them, and ``"gvis"`` (a tensor on
          this device, the result's shape) for G = 2 w (V - data).  Per time block ``SimHandle.run_residual`` fills a device
          block with G, then the handle passes the public functions run for the same outputs follow on it, with their
          accumulate rule: ``run_adjoint`` for ``gflux`` alone (``adjoint_path`` honoured; the only form a lattice handle
          takes), ``run_sky_adjoint`` for ``gflux`` with ``gtopo``, ``run_source_adjoint`` for ``gtopo`` alone,
          ``run_position_adjoint`` for ``gbls``; with ``beam_coefs`` ``run_basis_adjoint``, ``run_basis_position_adjoint``
          and ``run_basis_source_adjoint`` / ``run_sky_adjoint(basis=True)``, split as ``torch_simulate_vis_basis_sky``'s
          backward splits them.  The forward and the passes share the handle: with any output but ``gflux`` the lattice
          path is a ValueError (pass ``force_use_type3=True``).  Returns the (nfreqs, ntimes) float64 array of chi2 per
          (frequency, time) of the block.  An optional fourth element ``gains`` -- a host array (nfreqs, ntimes, nfeed,
          nant) of this precision's complex dtype, rows in ``ants``' order -- makes the data model
          ``conj(g[a1]) g[a2] V``: ``SimHandle.run_gain_residual`` replaces ``run_residual``, G is d chi2 / dV, and
          ``outputs["ggains"]`` (a host complex128 array of the gains' shape, optional) receives every block's rows of
          the gain gradient.  The fourth element ``("jones", block)`` -- ``block`` a host array (nfreqs, ntimes, 2, 2, nant)
          of this precision's complex dtype, ``block[f, t, i, j, a]`` the matrix of antenna ``a`` (``polarized=True``) --
          makes the data model ``A_a -> A_a block[a]`` instead: ``SimHandle.run_jones_residual`` runs per time block, and
          ``outputs["gjones"]`` (a host complex128 array of the block's shape, optional) receives the gradient rows.
        * ``gauss_newton_of`` (extra; what ``simulate_vis_gauss_newton`` passes): a triple ``(directions, weights, outputs)``
          -- the Gauss-Newton product H p, H = 2 J^T W J, from one handle and one set-up, the tangent U = J p never
          leaving the device.  ``directions`` is a dict, each entry optional, at least one given: ``"d_fluxes"`` (a host
          array of ``fluxes``' shape), ``"d_beam_coefs"`` ((1, nant, nbasis, nfreqs) complex; needs ``beam_coefs``),
          ``"d_baselines"`` ((nbls, 3) float64) and ``"d_topo"`` ((ntimes, nsrc, 3) float64), the last three numpy arrays
          or tensors on this device.  ``weights`` and ``outputs`` as for ``objective_of``; ``"gvis"`` receives
          G = 2 w U.  Per time block one device block per direction is filled, in this order: the forward
          (``SimHandle.run_device``) with the catalog's fluxes replaced by ``d_fluxes`` -- ``set_sources`` before and,
          with the real fluxes, after it, so every other pass sees the forward's --, ``run_basis_tangent``,
          ``run_tangent`` (``d_baselines`` and ``d_topo`` in one call) or with ``beam_coefs`` ``run_basis_position_tangent``,
          and with ``beam_coefs`` ``run_basis_source_tangent``.  ``SimHandle.weight_block`` sums them into G and the
          rows of sum w |U|^2, and ``objective_of``'s adjoint passes follow on G with its rules: the lattice path is
          taken by a call whose only direction is ``d_fluxes`` and whose only output is ``gflux`` (or none), a
          ValueError for any other on a lattice array (pass ``force_use_type3=True``).  Not with ``catalog_device``.
          Returns the (nfreqs, ntimes) float64 array of sum w |U|^2 per (frequency, time) of the block.  An optional
          fourth element ``(gains, d_gains)`` -- host arrays (nfreqs, ntimes, nfeed, nant) of this precision's complex
          dtype, rows in ``ants``' order, ``d_gains`` or None -- makes it the product of ``objective_of``'s chi2 with
          gains: the tangent is ``U' = m U + dm V``, ``SimHandle.gain_weight_block`` replaces ``weight_block``, G is
          ``conj(m) 2 w U'`` and the rows are sum w |U'|^2.  A gain direction counts as a direction (alone, no tangent
          pass runs), and ``outputs["ggains"]`` (a host complex128 array of the gains' shape, optional) receives the gain
          block of H p.  Only with ``d_gains`` or ``"ggains"`` one more block holds V, a forward run at the real fluxes.
          The lattice rule is unchanged: the product acts on the block whatever path produced it.  A fourth element
          ``("jones", (jones, d_jones))`` -- host arrays (nfreqs, ntimes, 2, 2, nant), ``d_jones`` or None; a polarized run
          -- makes it the product of ``objective_of``'s chi2 with Jones matrices under the same rules:
          ``SimHandle.jones_weight_block`` runs per time block and ``outputs["gjones"]`` receives the matrices' block of
          H p.
        * ``forward_to`` (extra; what ``simulate_vis_gain_solve`` passes): a C-contiguous tensor on this device of the
          result's shape and this run's complex dtype, or True for a new one.  The plain forward run fills it by pointer,
          time block by time block (``SimHandle.run_device``), and stays there: nothing comes to the host, and the tensor
          is returned.
        """
        name, payload = _which_pass(dict(
            adjoint_of=adjoint_of, tangent_of=tangent_of, basis_tangent_of=basis_tangent_of, basis_source_of=basis_source_of,
            sky_of=sky_of, objective_of=objective_of, gauss_newton_of=gauss_newton_of, forward_to=forward_to), out, out_shared)
        if adjoint_path not in ADJOINT_PATHS:
            raise ValueError(f"adjoint_path must be one of {ADJOINT_PATHS}, got {adjoint_path!r}")
        if adjoint_wrt not in _ADJOINT_WRT:
            raise ValueError(f"adjoint_wrt must be 'fluxes', 'positions' or 'sources', got {adjoint_wrt!r}")
        if name == "adjoint_of":  # three passes share the keyword
            name = _ADJOINT_WRT[adjoint_wrt]
        spec = _PASSES[name]
        if spec.needs_basis and beam_coefs is None:
            raise ValueError(f"{name} needs basis beams (beam_coefs)")
        if spec.check is not None:
            spec.check(payload, beam_coefs is not None)
        if spec.host_catalog and catalog_device is not None:
            raise ValueError(f"{name} does not take a device-resident catalog (catalog_device)")
        s = _host_setup(
            self.device, ants=ants, freqs=freqs, fluxes=fluxes, beam_list=beam_list, ra=ra, dec=dec, times=times,
            telescope_loc=telescope_loc, baselines=baselines, beam_idx=beam_idx, precision=precision, polarized=polarized,
            eps=eps, upsample_factor=upsample_factor, beam_spline_opts=beam_spline_opts, flat_array_tol=flat_array_tol,
            interpolation_function=interpolation_function, coord_method=coord_method, coord_method_params=coord_method_params,
            force_use_type3=force_use_type3, nchunks=nchunks, source_buffer=source_buffer, beam_coefs=beam_coefs,
            coord_mgr=coord_mgr, time_idx=time_idx, freq_idx=freq_idx, use_feed=use_feed, catalog_device=catalog_device,
            reference_compat=reference_compat, astrom=astrom, device_astrometry=device_astrometry)
        if s.is_gridded and spec.type3 is not None and spec.type3(payload):
            raise ValueError(f"{spec.refusal} the type-3 transform: pass force_use_type3=True on a lattice array")
        if adjoint_path == "type2" and not s.is_gridded:
            raise ValueError(
                "adjoint_path='type2' needs the lattice path: a flat, griddable array without force_use_type3 and "
                "without basis beams (adjoint_path='auto' falls back to the type-3 transform)")
        t0, t1, f0, f1 = s.span
        with _handle(self.device, precision, s.eps, upsample_factor, polarized) as h:
            _configure(h, s)
            if s.coord_mgr is not None:
                s.coord_mgr.setup()
            if spec.sets_adjoint_path and not s.use_basis:  # (a cached handle keeps its last setting)
                h.set_adjoint_path("type2" if s.is_gridded and adjoint_path != "type3" else "type3")
            if spec.prepare is not None:  # what of the payload needs the handle, or the device
                payload = spec.prepare(h, s, payload)
            # Walk the time axis in blocks whose output fits comfortably in free device memory (the
            # reference holds the whole (nt, nbls, nfeeds, nfeeds, nf) block in host RAM,
            # cpu_simulate.py:909-911); a coordinate manager's vectors are streamed block by block
            # instead of being stacked for all times on the host.  ``spec.blocks``: the blocks of the output's size
            # that the pass holds on the device per time step.
            nblk_t = _time_block(self.device, t1 - t0, int(np.ceil((f1 - f0) * spec.blocks(payload, s))), len(s.baselines),
                                 polarized, precision, s.nsrc if s.coord_mgr is not None else 0)
            return spec.run(h, s, payload, nblk_t)

    def _evaluate_vis_chunk(self, time_idx: slice, freq_idx: slice, **kw) -> np.ndarray:
        """One (time x freq) block in the reference's scratch layout
        (nt_here, nbls, nfeeds, nfeeds, nf_here) (reference cpu_simulate.py:909-911,1071).
        Takes the keyword arguments of ``simulate`` plus the block."""
        polarized = kw.get("polarized", False)
        final = self.simulate(time_idx=time_idx, freq_idx=freq_idx, **kw)
        if polarized:  # inverse of np.transpose(vis, (4, 0, 2, 3, 1)), cpu_simulate.py:851
            return np.transpose(final, (1, 4, 2, 3, 0))
        return np.moveaxis(final, 0, 2)[:, :, None, None, :]


def _host_setup(device, *, ants, freqs, fluxes, beam_list, ra, dec, times, telescope_loc, baselines, beam_idx, precision,
                polarized, eps, upsample_factor, beam_spline_opts, flat_array_tol, interpolation_function, coord_method,
                coord_method_params, force_use_type3, nchunks, source_buffer, beam_coefs, coord_mgr, time_idx, freq_idx,
                use_feed, catalog_device, reference_compat, astrom, device_astrometry):
    """``simulate``'s plain arguments, checked, as everything a handle will be told (``_configure``) and the loops need:
    one record.  Host work only: no handle, no device."""
    beam_order = checked_spline_order(beam_spline_opts)
    if interpolation_function not in ("az_za_map_coordinates", "az_za_simple"):
        raise ValueError(f"unknown interpolation_function {interpolation_function!r}")
    feed_index(use_feed)  # 'x' or 'y', else ValueError
    nchunks = int(nchunks)
    if nchunks < 1:
        raise ValueError("nchunks must be >= 1")
    if not 0.0 < float(source_buffer) <= 1.0:
        raise ValueError("source_buffer must be in (0, 1]")
    if astrom is None and device_astrometry and coord_mgr is None and coord_method != "SiderealRotation":
        from ..core.coords import erfa_astrom_context

        astrom = erfa_astrom_context(times, telescope_loc)
    if astrom is not None:
        astrom = np.ascontiguousarray(astrom, dtype=np.float64)
        if astrom.ndim != 2 or astrom.shape[1] != 31 or astrom.shape[0] != len(julian_dates(times)):
            raise ValueError("astrom must have shape (ntimes, 31): one eraASTROM context per time")
        if coord_mgr is not None:
            raise ValueError("pass either astrom= (device astrometry) or coord_mgr=, not both")
    if coord_mgr is None and astrom is None and coord_method != "SiderealRotation" and catalog_device is not None:
        raise ValueError(
            "a device-resident catalog carries no ra / dec for a matvis coordinate manager: pass coord_mgr= "
            "or coord_method='SiderealRotation'")
    freqs = np.asarray(freqs)
    nfreqs, ntimes, nbeam, nant = np.size(freqs), len(julian_dates(times)), len(beam_list), len(ants)
    real_dtype = np.float32 if precision == 1 else np.float64
    complex_dtype = np.complex64 if precision == 1 else np.complex128
    if eps is None:
        eps = default_accuracy_dict[precision]
    if upsample_factor == 1.25 and eps < (1e-8 if precision == 2 else 1e-4):
        # finufft's upsampfac = 1.25 has the same floor (its kernel width is capped likewise)
        warnings.warn(
            f"upsample_factor=1.25 delivers about {1e-8 if precision == 2 else 1e-4:g} at best "
            f"(eps={eps:g} was asked for); use upsample_factor=2 or 'auto' for tighter tolerances.",
            RuntimeWarning, stacklevel=3)  # (simulate's caller)
    # precision = 1 rounds ra/dec/freqs to float32 first (reference cpu_simulate.py:601-606)
    eq = coherency = polarized_sky = None
    if catalog_device is None:
        ra = np.asarray(ra).astype(real_dtype)
        dec = np.asarray(dec).astype(real_dtype)
        nsrc = int(ra.size)
    else:
        nsrc = int(catalog_device.nsrc)
    freqs = freqs.astype(real_dtype)
    ants = {k: np.asarray(v) for k, v in ants.items()}

    beam_idx = utils.validate_beam_idx(beam_idx, beam_coefs, nbeam, nant)
    if baselines is None:
        baselines = [red[0] for red in utils.get_pos_reds(ants, include_autos=True)]
    if catalog_device is None:
        coherency, polarized_sky = utils.prepare_source_catalog(np.asarray(fluxes), polarized)
        if coherency.shape[0] != nsrc or coherency.shape[1] != nfreqs:
            raise ValueError("fluxes must have shape (nsources, nfreqs[, 4])")
        eq = eq_unit_vectors(ra.astype(float), dec.astype(float))
    else:
        _check_device_catalog(catalog_device, nfreqs, polarized, precision, device)

    if coord_mgr is None and astrom is None and coord_method != "SiderealRotation":
        # the reference's own call (wrapper.py:308-336 passes no manager): build matvis' manager exactly
        # as the CPU engine does (cpu_simulate.py:686-709) and stream its vectors like a caller's
        coord_mgr = build_coord_mgr(coord_method, coord_method_params, coherency.astype(complex_dtype, copy=False),
                                    times, telescope_loc, ra, dec, precision, source_buffer, nchunks)

    # lattice arrays -> type 1 (reference cpu_simulate.py:634-637, 661-681)
    antvecs = np.array([ants[a] for a in ants], dtype=real_dtype)
    is_gridded = False
    if not force_use_type3 and beam_coefs is None and np.abs(antvecs[:, -1]).max() <= flat_array_tol:
        is_gridded, gridded_antpos, basis_matrix = check_antpos_griddability(ants)
    if is_gridded:
        bls_int = np.round(np.array(
            [gridded_antpos[bl[1]] - gridded_antpos[bl[0]] for bl in baselines]).T).astype(int)
        bls_int = bls_int.reshape(3, len(baselines))
        n_modes = 2 * int(np.round(np.max(np.abs(bls_int)))) + 1 if len(baselines) else 1
        array = ((basis_matrix / utils.speed_of_light).astype(real_dtype).astype(float), bls_int, n_modes)
    else:
        R, bls, is_coplanar = prepare_array(ants, baselines, flat_array_tol, real_dtype)
        array = (R.astype(float), bls.astype(float), is_coplanar)
    antnums = list(ants.keys())
    use_basis = beam_coefs is not None
    if use_basis:
        if not polarized:  # reference wrapper.py:280-283
            raise ValueError(
                "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to use beam_coefs."
            )
        beam_coefs = np.asarray(beam_coefs)
        if beam_coefs.shape != (nant, nbeam, nfreqs):
            raise ValueError("beam_coefs must have shape (nant, nbasis, nfreqs)")
        # per-baseline antenna rows of beam_coefs (reference cpu_simulate.py:920-921)
        beams = (beam_coefs, np.array([antnums.index(bl[0]) for bl in baselines]),
                 np.array([antnums.index(bl[1]) for bl in baselines]))
    else:
        beams = utils.prepare_beam_evaluation(antnums, baselines, beam_idx)  # (pairs, pair_idx, pair_flip)
    t0, t1, _ = time_idx.indices(ntimes)
    f0, f1, _ = freq_idx.indices(nfreqs)
    return types.SimpleNamespace(
        device=device, polarized=polarized, eps=eps, cdt=complex_dtype, nsrc=nsrc, nfreqs=nfreqs, nant=nant, antnums=antnums,
        baselines=baselines, span=(t0, t1, f0, f1),
        # the catalog: host arrays, or the device-resident one
        eq=eq, coherency=coherency, polarized_sky=polarized_sky, catalog_device=catalog_device,
        # the sources' directions per time: contexts, a manager's streamed vectors, or the sidereal rotations
        astrom=astrom, coord_mgr=coord_mgr,
        rotations=SiderealRotation(times, telescope_loc).matrices() if astrom is None and coord_mgr is None else None,
        freqs=freqs.astype(float),
        # set_array_type1's arguments on the lattice path (is_gridded), else set_array's
        is_gridded=is_gridded, array=array,
        beam_list=beam_list, beam_order=beam_order, use_feed=use_feed, nchunks=min(nchunks, max(nsrc, 1)),
        source_buffer=float(source_buffer), reference_compat=reference_compat,
        # set_basis' arguments with basis beams (use_basis), else set_beam_pairs'
        use_basis=use_basis, beams=beams)


def _configure(h, s):
    """Tell the handle ``h`` the run ``s`` (``_host_setup``'s record).  Every ``set_*`` fully replaces what it configures,
    so a cached handle serves any run of its creation parameters."""
    if s.catalog_device is None:
        h.set_sources(s.eq, s.coherency, s.polarized_sky)
    else:
        h.set_sources_device(s.nsrc, s.nfreqs, s.catalog_device.eq.data_ptr(), s.catalog_device.flux.data_ptr(),
                             s.catalog_device.polarized_sky)
    if s.astrom is not None:
        h.set_astrom(s.astrom)
    elif s.coord_mgr is None:
        h.set_times(s.rotations)
    h.set_freqs(s.freqs)
    if s.is_gridded:
        logger.info("Using gridded coordinates for the array. Type 1 transform will be used.")
        h.set_array_type1(*s.array)
    else:
        h.set_array(*s.array)
    h.set_beams(s.beam_list, s.freqs, s.beam_order, s.use_feed)
    h.set_chunking(s.nchunks, s.source_buffer)
    h.set_reference_compat(s.reference_compat)
    if s.use_basis:
        h.set_basis(*s.beams)
    else:
        h.set_beam_pairs(*s.beams)


@contextlib.contextmanager
def _handle(device, precision, eps, upsample_factor, polarized):
    """A handle for one run: back among the idle handles when the block ends, closed when it raises (an error may have
    left it half configured)."""
    key, h = _acquire_handle(device, precision, eps, upsample_factor, polarized)
    try:
        yield h
    except BaseException:
        h.close()
        raise
    _return_handle(key, h)


def build_coord_mgr(coord_method, coord_method_params, coherency, times, telescope_loc, ra, dec, precision,
                    source_buffer, nchunks):
    """The matvis coordinate manager the CPU engine builds at reference cpu_simulate.py:686-709, built the same
    way: ``CoordinateRotation._methods[coord_method](flux=, times=, telescope_loc=, skycoords=, precision=,
    source_buffer=, chunk_size=, **coord_method_params)``, BCRS fixed up front when ``update_bcrs_every``
    exceeds the observation's span.  matvis / astropy are imported here, on first use, because they are the
    reference's dependencies, not this backend's; without them the request is refused, never approximated."""
    try:
        from astropy import units as un
        from astropy.coordinates import SkyCoord
        from astropy.time import Time
        from matvis.core.coords import CoordinateRotation
    except ImportError as e:
        raise ValueError(
            f"coord_method={coord_method!r} needs matvis / astropy ({e}): install them (they are dependencies of "
            "fftvis), pass a matvis coordinate manager as coord_mgr= (its per-time topocentric vectors are used "
            "verbatim), or ask for the mean-sidereal approximation by name with coord_method='SiderealRotation' "
            "(no precession / nutation / aberration)") from e
    if coord_method not in CoordinateRotation._methods:
        raise ValueError(f"unknown coord_method {coord_method!r}")
    if isinstance(times, np.ndarray):  # cpu_simulate.py:686-687
        times = Time(times, format="jd")
    chunk_size = int(np.ceil(dec.size / nchunks))  # :689
    mgr = CoordinateRotation._methods[coord_method](
        flux=coherency,
        times=times,
        telescope_loc=telescope_loc,
        skycoords=SkyCoord(ra=ra * un.rad, dec=dec * un.rad, frame="icrs"),
        precision=precision,
        source_buffer=source_buffer,
        chunk_size=chunk_size,
        **(coord_method_params or {}),
    )
    if getattr(mgr, "update_bcrs_every", 0) > (times[-1] - times[0]).to(un.s):  # :706-709
        mgr._set_bcrs(0)
    return mgr


def _check_device_catalog(cat, nfreqs, polarized, precision, device):
    """Raw device pointers go to ``fv_sim_set_sources(on_device=1)``: everything the C side cannot see is
    checked here -- dtypes of the run's precision, contiguity, shapes, and the device the tensors live on."""
    import torch

    rdt = torch.float32 if precision == 1 else torch.float64
    cdt = torch.complex64 if precision == 1 else torch.complex128
    if cat.nfreq != nfreqs or (cat.polarized_sky and not polarized):
        raise ValueError("catalog_device does not match freqs / polarized")
    want_flux = (cat.nsrc, nfreqs, 2, 2) if cat.polarized_sky else (cat.nsrc, nfreqs)
    if tuple(cat.eq.shape) != (3, cat.nsrc) or tuple(cat.flux.shape) != want_flux:
        raise ValueError(f"catalog_device: eq must be (3, nsrc) and flux {want_flux}, got {tuple(cat.eq.shape)} / "
                         f"{tuple(cat.flux.shape)}")
    if cat.eq.dtype != rdt or cat.flux.dtype != (cdt if cat.polarized_sky else rdt):
        raise ValueError(f"catalog_device was built for another precision: eq {cat.eq.dtype}, flux {cat.flux.dtype}, "
                         f"run precision={precision}")
    if not (cat.eq.is_contiguous() and cat.flux.is_contiguous()):
        raise ValueError("catalog_device tensors must be contiguous")
    for t in (cat.eq, cat.flux):
        if t.device.type != "cuda" or (t.device.index or 0) != int(device):
            raise ValueError(f"catalog_device lives on {t.device}, the engine runs on cuda:{int(device)}")


def _topo_from_coord_mgr(coord_mgr, time_indices):
    """Topocentric unit vectors (len(time_indices), 3, nsrc) of every source at the given time indices
    from a matvis-style manager (``rotate(ti)``, attribute ``all_coords_topo``; ``setup()`` was called)."""
    out = []
    for ti in time_indices:
        coord_mgr.rotate(ti)
        out.append(np.array(coord_mgr.all_coords_topo, dtype=float))
    return np.stack(out)


def _time_blocks(h, t0, t1, nblk_t, coord_mgr):
    """The time blocks of a run, ``nblk_t`` steps each: yields (tb, te, ta, te_) -- the block [tb, te) of the time axis and
    the range [ta, te_) the handle ``h`` runs for it: the same, or with a coordinate manager (0, te - tb), after the
    block's vectors have been streamed to the handle (``set_topo``)."""
    step = max(nblk_t, 1)
    for tb in range(t0, t1, step):
        te = min(t1, tb + step)
        if coord_mgr is not None:
            h.set_topo(_topo_from_coord_mgr(coord_mgr, range(tb, te)))
            yield tb, te, 0, te - tb
        else:
            yield tb, te, tb, te


def _result_block(dv, axis, lo, hi, whole):
    """Where a run writes the steps [lo, hi) of ``dv``'s time ``axis``: ``dv`` itself when that is the whole result
    (returns (dv, None)), else a contiguous scratch block and the slice of ``dv`` it is copied to afterwards."""
    if whole:
        return dv, None
    dst = dv[(slice(None),) * axis + (slice(lo, hi),)]
    if isinstance(dv, np.ndarray):
        return np.empty(dst.shape, dtype=dv.dtype), dst
    import torch

    blk = torch.empty_like(dst, memory_format=torch.contiguous_format)
    torch.cuda.synchronize(blk.device)
    return blk, dst


def _block_input(x, lo, hi):
    """The time steps [lo, hi) (axis 1) of a pass's input ``x``, a numpy array or a tensor, as the library reads them:
    contiguous, and complete before the call that follows.  None stays None."""
    if x is None:
        return None
    blk = x[:, lo:hi]
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(blk)
    import torch

    blk = blk.contiguous()
    torch.cuda.synchronize(blk.device)  # a copy .contiguous() queued on torch's stream is done before the library reads
    return blk


def _run_forward(h, out, shared, t0, t1, f0, f1, nblk_t, coord_mgr):
    """The forward's time loop: one ``run`` when a block is the whole result and no coordinate manager streams its
    vectors, else every time block lands in its slice of the result (``fv_sim_run_into``): no block-sized temporary, no
    second host copy.  ``out``: the caller's array, or None for a new one."""
    if nblk_t >= t1 - t0 and coord_mgr is None:
        return h.run(t0, t1, f0, f1, out=out, shared=shared)
    vis = out if out is not None else np.empty(h.out_shape(t1 - t0, f1 - f0), dtype=h.cdt)
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        h.run(ta, te_, f0, f1, out=vis[:, tb - t0:te - t0], shared=shared)
    return vis


def _run_adjoint(h, g, gflux, t0, t1, f0, f1, nblk_t, coord_mgr, gcoefs=None, basis=False, positions=False, sources=False,
                 gbls=None):
    """The adjoint's time loop: the forward's blocks (and, with a coordinate manager, its streamed vectors), each block's
    contribution added to ``gflux`` (``basis``: and to ``gcoefs``; returns the pair -- with ``gbls`` the block's
    ``run_basis_position_adjoint`` follows and the triple is returned.  ``positions``: ``gflux`` is the
    (nbls, 3) baseline gradient and ``run_position_adjoint`` adds to it.  ``sources``: ``gflux`` is the (t1 - t0, nsrc, 3)
    direction gradient and every block's ``run_source_adjoint`` fills that block's rows).  Every ``run_adjoint`` call ends
    synchronised."""
    first = True
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        blk = _block_input(g, tb - t0, te - t0)
        if basis:
            if gflux is not None or gcoefs is not None:
                h.run_basis_adjoint(ta, te_, f0, f1, blk, gflux, gcoefs, not first)
            if gbls is not None:
                h.run_basis_position_adjoint(ta, te_, f0, f1, blk, gbls, not first)
        elif positions:
            h.run_position_adjoint(ta, te_, f0, f1, blk, gflux, not first)
        elif sources:  # (rows of a C-contiguous array: a contiguous view, written in place)
            h.run_source_adjoint(ta, te_, f0, f1, blk, gflux[tb - t0:te - t0], False)
        else:
            h.run_adjoint(ta, te_, f0, f1, blk, gflux, not first)
        first = False
    if first and not sources:  # no time steps: nothing contributes
        for out in (gflux, gcoefs, gbls):
            if out is not None:
                out[...] = 0
    if basis and gbls is not None:
        return gflux, gcoefs, gbls
    return (gflux, gcoefs) if basis else gflux


def _run_tangent(h, dbls, dtopo, dv, t0, t1, f0, f1, nblk_t, coord_mgr, basis=False):
    """The tangent's time loop: the forward's blocks (and, with a coordinate manager, its streamed vectors); every block's
    ``run_tangent`` takes its rows of ``dtopo`` and fills its slice of ``dv`` (a block that is not the whole result goes
    through a contiguous temporary).  ``basis``: ``run_basis_position_tangent`` on ``dbls``.  Every call ends synchronised."""
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        blk, dst = _result_block(dv, 1, tb - t0, te - t0, tb == t0 and te == t1)
        if basis:
            h.run_basis_position_tangent(ta, te_, f0, f1, dbls, blk)
        else:  # (rows of a C-contiguous array: a contiguous view)
            h.run_tangent(ta, te_, f0, f1, dbls, None if dtopo is None else dtopo[tb - t0:te - t0], blk)
        if dst is not None:
            dst[...] = blk
    if t1 <= t0:
        dv[...] = 0
    return dv


def _run_basis_source(h, mode, a, b, t0, t1, f0, f1, nblk_t, coord_mgr):
    """The time loop of the source passes through basis beams, over the forward's blocks (and, with a coordinate manager,
    its streamed vectors).  ``mode == "adjoint"``: ``a`` is g and every block's ``run_basis_source_adjoint`` fills that
    block's rows of ``b``, the (t1 - t0, nsrc, 3) direction gradient.  ``mode == "tangent"``: ``a`` is dtopo, and every
    block's ``run_basis_source_tangent`` takes its rows and fills its slice of ``b`` (a block that is not the whole result
    goes through a contiguous temporary).  Every call ends synchronised."""
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        if mode == "adjoint":
            h.run_basis_source_adjoint(ta, te_, f0, f1, _block_input(a, tb - t0, te - t0), b[tb - t0:te - t0], False)
        else:
            blk, dst = _result_block(b, 1, tb - t0, te - t0, tb == t0 and te == t1)
            h.run_basis_source_tangent(ta, te_, f0, f1, a[tb - t0:te - t0], blk)
            if dst is not None:
                dst[...] = blk
    if t1 <= t0 and mode == "tangent":
        b[...] = 0
    return b


def _run_sky_adjoint(h, g, gflux, gtopo, t0, t1, f0, f1, nblk_t, coord_mgr, basis=False):
    """The joint sky adjoint's time loop, over the forward's blocks (and, with a coordinate manager, its streamed vectors):
    every block's ``run_sky_adjoint`` adds its contribution to ``gflux`` -- the first block overwrites -- and fills its rows
    of ``gtopo``, the (t1 - t0, nsrc, 3) direction gradient.  The two outputs share one ``accumulate`` flag, so a later
    block adds to its rows of the caller's zeroed buffer.  Every call ends synchronised."""
    first = True
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        blk = _block_input(g, tb - t0, te - t0)
        # (rows of a C-contiguous array: a contiguous view, written in place)
        h.run_sky_adjoint(ta, te_, f0, f1, blk, gflux, gtopo[tb - t0:te - t0], not first, basis=basis)
        first = False
    if first:  # no time steps: nothing contributes
        gflux[...] = 0
    return gflux, gtopo


_OBJECTIVE_OUTPUTS = ("gflux", "gcoefs", "gbls", "gtopo", "gvis")
_GAIN_OUTPUT = "ggains"  # (objective_of with gains only)
_JONES_OUTPUT = "gjones"  # (objective_of with Jones matrices only)


def _is_jones(gains):
    """Whether the fourth element of ``objective_of`` holds Jones matrices: ``("jones", block)``, which no array of gains
    can be mistaken for."""
    return isinstance(gains, tuple) and len(gains) == 2 and isinstance(gains[0], str) and gains[0] == "jones"


def _run_objective(h, device, data, weights, outputs, t0, t1, f0, f1, nblk_t, coord_mgr, basis=False, gains=None):
    """The fused objective's time loop, over the forward's blocks (and, with a coordinate manager, its streamed vectors):
    every block's ``run_residual`` leaves G = 2 w (V - data) in a device block -- ``outputs["gvis"]`` itself when one block
    is the whole result -- and its rows of chi2; the handle passes for the outputs given follow on that block as
    ``_run_adjoint``, ``_run_sky_adjoint`` and ``_run_basis_source`` run them: the first block overwrites ``gflux``,
    ``gcoefs`` and ``gbls``, later ones add, and every block fills its rows of ``gtopo``.  With ``gains`` (host, (f1 - f0,
    t1 - t0, nfeed, nant)) every block's ``run_gain_residual`` takes its time steps of them instead and fills its time
    steps of ``outputs["ggains"]``; the passes read its G unchanged.  With ``gains = ("jones", block)`` (host, (f1 - f0,
    t1 - t0, 2, 2, nant)) it is ``run_jones_residual`` and ``outputs["gjones"]``.  Returns chi2, (f1 - f0, t1 - t0) float64
    on the host.  Every call ends synchronised."""
    jones = _is_jones(gains)
    if jones:
        gains = gains[1]
    ggains = outputs.get(_JONES_OUTPUT if jones else _GAIN_OUTPUT)
    chi2 = np.zeros((f1 - f0, t1 - t0), dtype=np.float64)
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        lo, hi = tb - t0, te - t0
        g, = _device_blocks(h, device, 1, outputs, lo, hi, t1 - t0, f1 - f0)
        d, w = _block_input(data, lo, hi), _block_input(weights, lo, hi)
        if gains is None:
            chi2[:, lo:hi] = h.run_residual(ta, te_, f0, f1, d, w, g)
        else:
            gg = _gain_output_block(ggains, lo, hi)
            residual = h.run_jones_residual if jones else h.run_gain_residual
            chi2[:, lo:hi] = residual(ta, te_, f0, f1, d, w, _block_input(gains, lo, hi), g, gg)
            if gg is not None:
                ggains[:, lo:hi] = gg
        _adjoints_of_block(h, g, outputs, lo, hi, t1 - t0, ta, te_, f0, f1, basis)
    return chi2


def _device_blocks(h, device, n, outputs, lo, hi, nt, nf):
    """``n`` device blocks for the time steps [lo, hi) of a fit pass (``_run_objective``, ``_run_gauss_newton``), each a new
    C-contiguous tensor of ``out_shape(hi - lo, nf)`` in the handle's complex dtype -- but the first, which receives G, is
    ``outputs["gvis"]`` itself when that is given and the block is the whole result of ``nt`` steps.  Complete before the
    library writes them."""
    import torch

    dev = torch.device("cuda", int(device))
    whole_gvis = outputs.get("gvis") if (lo, hi) == (0, nt) else None
    blocks = [torch.empty(h.out_shape(hi - lo, nf), dtype=getattr(torch, np.dtype(h.cdt).name), device=dev)
              for _ in range(n - int(whole_gvis is not None))]
    torch.cuda.synchronize(dev)
    return blocks if whole_gvis is None else [whole_gvis] + blocks


def _gain_output_block(ggains, lo, hi):
    """A contiguous host block for the time steps [lo, hi) of the gain output ``ggains`` (complex128, the gains' block
    layout), which the caller copies to ``ggains[:, lo:hi]`` once the library has filled it; None stays None."""
    return None if ggains is None else np.empty(ggains[:, lo:hi].shape, dtype=np.complex128)


def _adjoints_of_block(h, g, outputs, lo, hi, nt, ta, te_, f0, f1, basis):
    """What follows G of the time steps [lo, hi) out of ``nt``, in the device block ``g`` (``_run_objective``,
    ``_run_gauss_newton``): its copy into ``outputs["gvis"]`` unless ``g`` is that tensor, then the handle passes for the
    outputs given, which take the block's rows of ``gtopo``; the first block overwrites the other outputs, later ones add."""
    gflux, gcoefs, gbls, gtopo, gvis = (outputs.get(k) for k in _OBJECTIVE_OUTPUTS)
    if gvis is not None and g is not gvis:
        import torch

        gvis[:, lo:hi] = g
        torch.cuda.synchronize(g.device)
    first = lo == 0
    rows = None if gtopo is None else gtopo[lo:hi]  # (rows of a C-contiguous array: a contiguous view)
    if gflux is not None and rows is not None:  # one pass for both
        h.run_sky_adjoint(ta, te_, f0, f1, g, gflux, rows, not first, basis=basis)
        if gcoefs is not None:
            h.run_basis_adjoint(ta, te_, f0, f1, g, None, gcoefs, not first)
    elif basis:
        if gflux is not None or gcoefs is not None:
            h.run_basis_adjoint(ta, te_, f0, f1, g, gflux, gcoefs, not first)
        if rows is not None:
            h.run_basis_source_adjoint(ta, te_, f0, f1, g, rows, False)
    elif gflux is not None:
        h.run_adjoint(ta, te_, f0, f1, g, gflux, not first)
    elif rows is not None:
        h.run_source_adjoint(ta, te_, f0, f1, g, rows, False)
    if gbls is not None:
        if basis:
            h.run_basis_position_adjoint(ta, te_, f0, f1, g, gbls, not first)
        else:
            h.run_position_adjoint(ta, te_, f0, f1, g, gbls, not first)


_GAUSS_NEWTON_DIRECTIONS = ("d_fluxes", "d_beam_coefs", "d_baselines", "d_topo")


def _gauss_newton_nparts(directions, basis):
    """Device blocks a time block of the Gauss-Newton product holds, one per tangent pass: without basis beams
    ``d_baselines`` and ``d_topo`` share one."""
    given = [directions.get(k) is not None for k in _GAUSS_NEWTON_DIRECTIONS]
    return sum(given) if basis else int(given[0]) + int(given[2] or given[3])


def _gauss_newton_holds_v(outputs, gains):
    """Whether a time block of the Gauss-Newton product holds V in one more device block: only with a gain direction or
    the gain block of H p as an output.  ``gains``: (gains, d_gains), ("jones", (jones, d_jones)) or None."""
    if _is_jones(gains):
        return gains[1][1] is not None or outputs.get(_JONES_OUTPUT) is not None
    return gains is not None and (gains[1] is not None or outputs.get(_GAIN_OUTPUT) is not None)


def _run_gauss_newton(h, device, directions, weights, outputs, set_fluxes, t0, t1, f0, f1, nblk_t, coord_mgr, basis=False,
                      gains=None):
    """The Gauss-Newton product's time loop, over the forward's blocks (and, with a coordinate manager, its streamed
    vectors).  Per block one device block per tangent pass, filled by pointer in this order: the forward on ``d_fluxes``
    (``set_fluxes(True)`` before, ``set_fluxes(False)`` after: every other pass sees the real fluxes), ``run_basis_tangent``
    on ``d_beam_coefs``, the position tangent on ``d_baselines`` (without basis beams ``d_topo`` rides in the same
    ``run_tangent``), ``run_basis_source_tangent`` on ``d_topo``.  ``weight_block`` leaves G = 2 w (their sum) in the first
    -- ``outputs["gvis"]`` itself when one block is the whole result -- and the block's rows of sum w |U|^2; the adjoint
    passes follow on G as in ``_run_objective``.  With ``gains = (gains, d_gains)`` (host, (f1 - f0, t1 - t0, nfeed, nant);
    ``d_gains`` or None) ``gain_weight_block`` takes the block's time steps of them instead, G is ``conj(m) 2 w U'`` and the
    rows are sum w |U'|^2; only with ``d_gains`` or ``outputs["ggains"]`` one more block is filled with V -- ``run_device``
    at the real fluxes, after the parts -- and the block's time steps of ``ggains`` are filled; without a sky direction V's
    block receives G.  With ``gains = ("jones", (jones, d_jones))`` (host, (f1 - f0, t1 - t0, 2, 2, nant)) it is
    ``jones_weight_block`` and ``outputs["gjones"]``, under the same rules.  Returns the rows, (f1 - f0, t1 - t0) float64 on
    the host.  Every call ends synchronised."""
    hold_v = _gauss_newton_holds_v(outputs, gains)
    jones = _is_jones(gains)
    if jones:
        gains = gains[1]
    ggains = outputs.get(_JONES_OUTPUT if jones else _GAIN_OUTPUT)
    d_fluxes, d_coefs, d_bls, d_topo = (directions.get(k) for k in _GAUSS_NEWTON_DIRECTIONS)
    nparts = _gauss_newton_nparts(directions, basis)
    quad = np.zeros((f1 - f0, t1 - t0), dtype=np.float64)
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        lo, hi = tb - t0, te - t0
        # (block 0 receives G: the first part, or V for a gains-only direction)
        parts = _device_blocks(h, device, nparts + int(hold_v), outputs, lo, hi, t1 - t0, f1 - f0)
        vis = parts.pop(0 if nparts == 0 else -1) if hold_v else None
        rows_in = None if d_topo is None else d_topo[lo:hi]  # (rows of a C-contiguous array: a contiguous view)
        todo = iter(parts)
        if d_fluxes is not None:
            set_fluxes(True)
            h.run_device(ta, te_, f0, f1, next(todo).data_ptr())
            h.sync()  # (run_device only queues: the forward has read the direction before the real fluxes come back)
            set_fluxes(False)
        if d_coefs is not None:
            h.run_basis_tangent(ta, te_, f0, f1, d_coefs, next(todo))
        if basis:
            if d_bls is not None:
                h.run_basis_position_tangent(ta, te_, f0, f1, d_bls, next(todo))
            if d_topo is not None:
                h.run_basis_source_tangent(ta, te_, f0, f1, rows_in, next(todo))
        elif d_bls is not None or d_topo is not None:
            h.run_tangent(ta, te_, f0, f1, d_bls, rows_in, next(todo))
        if hold_v:  # (the real fluxes are back)
            h.run_device(ta, te_, f0, f1, vis.data_ptr())
        w = _block_input(weights, lo, hi)
        if gains is None:
            quad[:, lo:hi] = h.weight_block(ta, te_, f0, f1, parts, w)
        else:
            hg = _gain_output_block(ggains, lo, hi)
            weight = h.jones_weight_block if jones else h.gain_weight_block
            quad[:, lo:hi] = weight(ta, te_, f0, f1, parts, vis, w, _block_input(gains[0], lo, hi),
                                    _block_input(gains[1], lo, hi), hg)
            if hg is not None:
                ggains[:, lo:hi] = hg
        _adjoints_of_block(h, parts[0] if parts else vis, outputs, lo, hi, t1 - t0, ta, te_, f0, f1, basis)
    return quad


def _forward_target(h, device, vis, nt, nf):
    """``forward_to`` as the tensor the forward fills: the caller's, checked, or for True a new one.  It holds the whole
    (nf, nt, ...) result, so it is made before the time blocks are sized: ``_time_block`` then sees the memory left."""
    import torch

    cdt = getattr(torch, np.dtype(h.cdt).name)
    if vis is True:
        vis = torch.empty(h.out_shape(nt, nf), dtype=cdt, device=torch.device("cuda", int(device)))
        torch.cuda.synchronize(vis.device)
    if (not isinstance(vis, torch.Tensor) or vis.device != torch.device("cuda", int(device)) or vis.dtype != cdt
            or tuple(vis.shape) != h.out_shape(nt, nf) or not vis.is_contiguous()):
        raise ValueError(f"forward_to must be a C-contiguous {np.dtype(h.cdt).name} tensor on cuda:{int(device)} of shape "
                         f"{h.out_shape(nt, nf)}")
    return vis


def _run_forward_to(h, vis, t0, t1, f0, f1, nblk_t, coord_mgr):
    """The forward run into the device tensor ``vis`` (``_forward_target``'s): the forward's time blocks (and, with a
    coordinate manager, its streamed vectors); every block's ``run_device`` fills its slice ``vis[:, block]`` (a block
    that is not the whole result goes through a contiguous temporary).  Every call ends synchronised."""
    import torch

    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        blk, dst = _result_block(vis, 1, tb - t0, te - t0, tb == t0 and te == t1)
        torch.cuda.synchronize(vis.device)
        h.run_device(ta, te_, f0, f1, blk.data_ptr())
        h.sync()  # (run_device only queues)
        if dst is not None:
            dst[...] = blk
            torch.cuda.synchronize(vis.device)
    return vis


def _run_basis_tangent(h, dcoefs, dv, t0, t1, f0, f1, nblk_t, coord_mgr):
    """The basis tangent's time loop: the forward's blocks (and, with a coordinate manager, its streamed vectors); every
    block's ``run_basis_tangent`` fills its slice ``dv[:, :, block]`` of every direction (a block that is not the whole
    result goes through a contiguous temporary).  Every call ends synchronised."""
    for tb, te, ta, te_ in _time_blocks(h, t0, t1, nblk_t, coord_mgr):
        blk, dst = _result_block(dv, 2, tb - t0, te - t0, tb == t0 and te == t1)
        h.run_basis_tangent(ta, te_, f0, f1, dcoefs, blk)
        if dst is not None:
            dst[...] = blk
    if t1 <= t0:
        dv[...] = 0
    return dv


# ---- the passes of ``simulate``: which one a call asks for, and what ``simulate`` has to know about each ----

# the mode keywords, in the order they were added: two of them in one call are refused in the name of the later one
_MODES = ("adjoint_of", "tangent_of", "basis_tangent_of", "basis_source_of", "sky_of", "objective_of", "gauss_newton_of",
          "forward_to")
_ADJOINT_WRT = {"fluxes": "adjoint_of", "positions": "position_adjoint", "sources": "source_adjoint"}  # adjoint_of's passes


def _which_pass(modes: dict, out, out_shared):
    """(name, payload) of the pass a call asks for: the one mode keyword given (``modes``: every keyword of ``_MODES`` with
    its value) with its value, or ("forward", (out, out_shared)).  ValueError for more than one."""
    given = [k for k in _MODES if modes[k] is not None]
    if "forward_to" in given and (len(given) > 1 or out is not None):
        raise ValueError("forward_to is the plain forward run: no other pass and no out= with it")
    if len(given) > 1:
        earlier = _MODES[:_MODES.index(given[-1])]
        if len(earlier) == 1:
            raise ValueError(f"pass either {earlier[0]} or {given[-1]}, not both")
        raise ValueError(f"pass one of {', '.join(earlier)} and {given[-1]}")
    return (given[0], modes[given[0]]) if given else ("forward", (out, out_shared))


def _check_adjoint(p, basis):
    if basis != (len(p) in (3, 4)):
        raise ValueError("adjoint_of: (g, gflux, gcoefs[, gbls]) with beam_coefs, (g, gflux) without")


def _no_basis_beams(what):
    def check(p, basis):
        if basis:
            raise ValueError(f"the {what} adjoint does not cover basis beams (beam_coefs)")
        _check_adjoint(p, basis)
    return check


def _check_tangent(p, basis):
    if basis and (p[1] is not None or p[0] is None):
        raise ValueError("the tangent through basis beams (beam_coefs) takes baseline directions only: source "
                         "directions are not covered")


def _check_basis_source(p, basis):
    if len(p) != 3 or p[0] not in ("adjoint", "tangent"):
        raise ValueError("basis_source_of: ('adjoint', g, gtopo) or ('tangent', dtopo, dv)")


def _check_sky(p, basis):
    if len(p) != 3:
        raise ValueError("sky_of: (g, gflux, gtopo)")


def _check_objective(p, basis):
    if (len(p) not in (3, 4) or not isinstance(p[2], dict)
            or set(p[2]) - set(_OBJECTIVE_OUTPUTS) - {_GAIN_OUTPUT, _JONES_OUTPUT}):
        raise ValueError(f"objective_of: (data, weights, outputs) with outputs a dict over {_OBJECTIVE_OUTPUTS}")
    if p[2].get("gcoefs") is not None and not basis:
        raise ValueError("objective_of: gcoefs needs basis beams (beam_coefs)")
    fourth = p[3] if len(p) == 4 else None
    if isinstance(fourth, tuple) and not _is_jones(fourth):
        raise ValueError("objective_of: the fourth element is the gains, or ('jones', block)")
    if p[2].get(_GAIN_OUTPUT) is not None and (fourth is None or _is_jones(fourth)):
        raise ValueError("objective_of: ggains needs the gains (a fourth element)")
    if p[2].get(_JONES_OUTPUT) is not None and not _is_jones(fourth):
        raise ValueError("objective_of: gjones needs the matrices (a fourth element ('jones', block))")


def _check_gauss_newton(p, basis):
    if (len(p) not in (3, 4) or not isinstance(p[0], dict) or not isinstance(p[2], dict)
            or set(p[0]) - set(_GAUSS_NEWTON_DIRECTIONS)
            or set(p[2]) - set(_OBJECTIVE_OUTPUTS) - {_GAIN_OUTPUT, _JONES_OUTPUT}):
        raise ValueError(f"gauss_newton_of: (directions, weights, outputs) with directions a dict over "
                         f"{_GAUSS_NEWTON_DIRECTIONS} and outputs a dict over {_OBJECTIVE_OUTPUTS}")
    gains = p[3] if len(p) == 4 else None
    jones = _is_jones(gains)
    if jones:  # (the same pair, tagged)
        gains = gains[1]
    if gains is not None and (not isinstance(gains, tuple) or len(gains) != 2 or gains[0] is None):
        raise ValueError("gauss_newton_of: the fourth element is (gains, d_gains), d_gains or None"
                         + (", tagged ('jones', (jones, d_jones)) for Jones matrices" if jones else ""))
    if p[2].get(_GAIN_OUTPUT) is not None and (gains is None or jones):
        raise ValueError("gauss_newton_of: ggains needs the gains (a fourth element)")
    if p[2].get(_JONES_OUTPUT) is not None and not jones:
        raise ValueError("gauss_newton_of: gjones needs the matrices (a fourth element ('jones', (jones, d_jones)))")
    if all(p[0].get(k) is None for k in _GAUSS_NEWTON_DIRECTIONS) and (gains is None or gains[1] is None):
        raise ValueError("gauss_newton_of: no direction given")
    if not basis and (p[0].get("d_beam_coefs") is not None or p[2].get("gcoefs") is not None):
        raise ValueError("gauss_newton_of: d_beam_coefs and gcoefs need basis beams (beam_coefs)")


def _position_outputs(outputs):
    return any(outputs.get(k) is not None for k in ("gcoefs", "gbls", "gtopo"))


def _prepare_forward(h, s, p):
    t0, t1, f0, f1 = s.span
    out = p[0]
    if out is not None and (out.shape != h.out_shape(t1 - t0, f1 - f0) or out.dtype != s.cdt):
        raise ValueError(f"out must be a {np.dtype(s.cdt).name} array of shape "
                         f"{h.out_shape(t1 - t0, f1 - f0)}, got {out.dtype} {out.shape}")
    return p


def _set_gain_pairs(h, s, keyword, named_gains, jones=False):
    """The fit passes' gains: every block of ``named_gains`` -- (name, host array or None) -- checked against the run's
    (nf, nt, nfeed, nant) layout -- (nf, nt, 2, 2, nant) for Jones matrices --, then the antenna pair of every baseline, as
    rows of ``ants``' order, told to the handle."""
    t0, t1, f0, f1 = s.span
    shape = (f1 - f0, t1 - t0) + ((2, 2) if jones else (2 if s.polarized else 1,)) + (s.nant,)
    for name, x in named_gains:
        if x is not None and (not isinstance(x, np.ndarray) or x.dtype != s.cdt or x.shape != shape):
            raise ValueError(f"{keyword}: {name} must be a {np.dtype(s.cdt).name} array of shape {shape}")
    row = {a: i for i, a in enumerate(s.antnums)}  # (list.index per baseline is 0.2 s at HERA-350's 61 075)
    nb = len(s.baselines)
    h.set_gain_pairs(s.nant, np.fromiter((row[bl[0]] for bl in s.baselines), np.int32, count=nb),
                     np.fromiter((row[bl[1]] for bl in s.baselines), np.int32, count=nb))


def _prepare_objective(h, s, p):
    """``objective_of`` as (data, weights, outputs, gains, ("jones", block) or None), the handle told the gain pairs."""
    gains = p[3] if len(p) == 4 else None
    if _is_jones(gains):
        if not s.polarized:
            raise ValueError("objective_of: Jones matrices need polarized=True")
        _set_gain_pairs(h, s, "objective_of", [("jones", gains[1])], jones=True)
    elif gains is not None:
        _set_gain_pairs(h, s, "objective_of", [("gains", gains)])
    return p[0], p[1], p[2], gains


def _prepare_gauss_newton(h, s, p):
    """``gauss_newton_of`` as (directions, weights, outputs, set_fluxes, (gains, d_gains) or None), the handle told the
    gain pairs.  ``set_fluxes(tangent)`` (None without ``d_fluxes``) sets the catalog's fluxes: the direction's for the
    forward part, else the real ones."""
    directions, gains = p[0], p[3] if len(p) == 4 else None
    set_fluxes = None
    if directions.get("d_fluxes") is not None:
        d_coherency, _ = utils.prepare_source_catalog(np.asarray(directions["d_fluxes"]), s.polarized)
        if d_coherency.shape != s.coherency.shape:  # (the same shape: the same kind of sky)
            raise ValueError(f"d_fluxes must have fluxes' shape, got {np.shape(directions['d_fluxes'])}")

        def set_fluxes(tangent):
            h.set_sources(s.eq, d_coherency if tangent else s.coherency, s.polarized_sky)
    if _is_jones(gains):
        if not s.polarized:
            raise ValueError("gauss_newton_of: Jones matrices need polarized=True")
        _set_gain_pairs(h, s, "gauss_newton_of", zip(("jones", "d_jones"), gains[1]), jones=True)
    elif gains is not None:
        _set_gain_pairs(h, s, "gauss_newton_of", zip(("gains", "d_gains"), gains))
    return directions, p[1], p[2], set_fluxes, gains


def _prepare_forward_to(h, s, p):
    # (the target holds the whole model: made before the time blocks are sized, so that a block's temporary fits next to it)
    return _forward_target(h, s.device, p, s.span[1] - s.span[0], s.span[3] - s.span[2])


class _Pass(typing.NamedTuple):
    """What ``simulate`` has to know about one pass.  ``p`` is the pass's payload -- its mode keyword's value, or what
    ``prepare`` made of it --, ``s`` the run (``_host_setup``'s record), ``h`` the configured handle."""

    run: typing.Callable  # (h, s, p, nblk_t) -> the call's result: the pass's time loop
    check: typing.Callable = None  # (p, basis): ValueError for a payload the pass does not take, before any set-up
    needs_basis: bool = False  # refused without beam_coefs
    host_catalog: bool = False  # refused with catalog_device
    type3: typing.Callable = None  # (p) -> whether the pass, given its payload, runs the type-3 transform only ...
    refusal: str = None  # ... and how its refusal of a lattice array begins
    sets_adjoint_path: bool = False  # adjoint_path is told to the handle (no basis beams)
    prepare: typing.Callable = None  # (h, s, p) -> p: the checks and the set-up of the payload that need the handle
    blocks: typing.Callable = lambda p, s: 1  # (p, s) -> device blocks of the output's size a time step holds


def _always(p):
    return True


_PASSES = {
    "forward": _Pass(
        run=lambda h, s, p, n: _run_forward(h, p[0], p[1], *s.span, n, s.coord_mgr), prepare=_prepare_forward),
    "adjoint_of": _Pass(
        run=lambda h, s, p, n: _run_adjoint(h, p[0], p[1], *s.span, n, s.coord_mgr, gcoefs=p[2] if s.use_basis else None,
                                            basis=s.use_basis, gbls=p[3] if len(p) == 4 else None),
        check=_check_adjoint, sets_adjoint_path=True),
    "position_adjoint": _Pass(
        run=lambda h, s, p, n: _run_adjoint(h, p[0], p[1], *s.span, n, s.coord_mgr, positions=True),
        check=_no_basis_beams("position"), type3=_always, refusal="the position adjoint runs", sets_adjoint_path=True),
    "source_adjoint": _Pass(
        run=lambda h, s, p, n: _run_adjoint(h, p[0], p[1], *s.span, n, s.coord_mgr, sources=True),
        check=_no_basis_beams("source"), type3=_always, refusal="the source adjoint runs", sets_adjoint_path=True),
    "tangent_of": _Pass(
        run=lambda h, s, p, n: _run_tangent(h, p[0], p[1], p[2], *s.span, n, s.coord_mgr, basis=s.use_basis),
        check=_check_tangent, type3=_always, refusal="the tangent runs"),
    "basis_tangent_of": _Pass(
        run=lambda h, s, p, n: _run_basis_tangent(h, p[0], p[1], *s.span, n, s.coord_mgr), needs_basis=True,
        blocks=lambda p, s: int(p[0].shape[0])),  # (the device holds every direction's copy of a time block)
    "basis_source_of": _Pass(
        run=lambda h, s, p, n: _run_basis_source(h, *p, *s.span, n, s.coord_mgr), check=_check_basis_source,
        needs_basis=True),
    "sky_of": _Pass(
        run=lambda h, s, p, n: _run_sky_adjoint(h, *p, *s.span, n, s.coord_mgr, basis=s.use_basis), check=_check_sky,
        type3=_always, refusal="the sky adjoint runs"),
    # (a block's G, data and weights are on the device together: 2.5 blocks, 2 without weights; a block's gains and their
    # gradient add (8 + 16) nfeed nant bytes per row to the 2.5 blocks of 8 tpol nbls: under 0.1 % once nbls >= nant; Jones
    # matrices add the rows' fp64 terms, 8 bytes per value: half a block in fp64, a whole one in fp32)
    "objective_of": _Pass(
        run=lambda h, s, p, n: _run_objective(h, s.device, p[0], p[1], p[2], *s.span, n, s.coord_mgr, basis=s.use_basis,
                                              gains=p[3]),
        check=_check_objective, type3=lambda p: _position_outputs(p[2]), refusal="the objective's position passes run",
        sets_adjoint_path=True, prepare=_prepare_objective,
        blocks=lambda p, s: (2.0 if p[1] is None else 2.5) + (8.0 / np.dtype(s.cdt).itemsize if _is_jones(p[3]) else 0.0)),
    # (a block's parts and weights are on the device together: one block per part, half a block of weights, one more
    # block when V is held; the gains, their direction and the product are under 0.1 % of one; Jones matrices add the rows'
    # fp64 terms as in objective_of)
    "gauss_newton_of": _Pass(
        run=lambda h, s, p, n: _run_gauss_newton(h, s.device, p[0], p[1], p[2], p[3], *s.span, n, s.coord_mgr,
                                                 basis=s.use_basis, gains=p[4]),
        check=_check_gauss_newton, host_catalog=True,
        type3=lambda p: (any(p[0].get(k) is not None for k in ("d_beam_coefs", "d_baselines", "d_topo"))
                         or _position_outputs(p[2])),
        refusal="the Gauss-Newton product's position passes run", sets_adjoint_path=True, prepare=_prepare_gauss_newton,
        blocks=lambda p, s: (_gauss_newton_nparts(p[0], s.use_basis) + (0.0 if p[1] is None else 0.5)
                             + (1.0 if _gauss_newton_holds_v(p[2], p[4]) else 0.0)
                             + (8.0 / np.dtype(s.cdt).itemsize if _is_jones(p[4]) else 0.0))),
    "forward_to": _Pass(
        run=lambda h, s, p, n: _run_forward_to(h, p, *s.span, n, s.coord_mgr), prepare=_prepare_forward_to),
}


def _time_block(device, nt, nf, nbls, polarized, precision, nsrc_topo=0):
    """Time steps per fv_sim_run: as many as keep the output block under 45 % of free device memory
    (and, with a coordinate manager, the staged vectors of a block under 2 GiB)."""
    from ..wrapper import device_memory_budget  # free + what this process's own cached handles hold

    per_time = max(1, nf * nbls * (4 if polarized else 1) * 8 * precision)
    n = max(1, int(0.45 * device_memory_budget(device) // per_time))
    if nsrc_topo:
        n = min(n, max(1, int(2**31 // (3 * nsrc_topo * 4 * precision))))
    return min(n, max(nt, 1))


if "fftvis.core.simulate" in __import__("sys").modules:
    register_with_reference()
