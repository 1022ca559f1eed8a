"""References of the Gauss-Newton product (``simulate_vis_gauss_newton``, ``fv_sim_weight_block``, ``fv_weight_rows``) in
numpy."""

import numpy as np


def weight_rows(parts, w=None):
    """(G, U, terms) as the kernel forms them for part blocks of one precision T: ``U = ((P_0 + P_1) + P_2) + P_3`` added
    component-wise in T in that order, ``G = 2 (w U)`` with ``w re`` and ``w im`` rounded separately in T and doubled
    exactly, and the fp64 terms ``w |U|^2`` of the rows' sums.  ``w`` None means 1; where ``w == 0`` the sample is flagged:
    G is 0, the term is 0 and the parts are not used (they may be NaN)."""
    cdt = parts[0].dtype
    rdt = parts[0].real.dtype
    re, im = parts[0].real.copy(), parts[0].imag.copy()
    for p in parts[1:]:
        assert p.dtype == cdt
        with np.errstate(invalid="ignore"):
            re, im = (re + p.real).astype(rdt), (im + p.imag).astype(rdt)
    w = np.ones(re.shape, dtype=rdt) if w is None else np.asarray(w, dtype=rdt)
    used = w != 0
    re, im = np.where(used, re, 0).astype(rdt), np.where(used, im, 0).astype(rdt)
    G = np.empty(re.shape, dtype=cdt)
    G.real = (rdt.type(2) * (w * re).astype(rdt)).astype(rdt)
    G.imag = (rdt.type(2) * (w * im).astype(rdt)).astype(rdt)
    U = np.empty(re.shape, dtype=cdt)
    U.real, U.imag = re, im
    terms = w.astype(np.float64) * (re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)
    return G, U, terms


def quad_and_gvis(U, w=None):
    """(quad_rows, G) in fp64 for a tangent block whose rows are the leading two axes (frequency, time):
    ``quad_rows = sum over the row of w |U|^2`` and ``G = 2 w U``; ``w`` None means 1, and where ``w == 0`` U is not used."""
    U = np.asarray(U, dtype=np.complex128)
    w = np.ones(U.shape) if w is None else np.asarray(w, dtype=np.float64)
    U = np.where(w != 0, U, 0)
    terms = w * (U.real**2 + U.imag**2)
    return terms.reshape(U.shape[:2] + (-1,)).sum(axis=-1), 2 * w * U


def inner(d, prod):
    """``Re <d, prod>`` in fp64 -- the real dot product for real arrays."""
    d, prod = np.asarray(d), np.asarray(prod)
    return float(np.sum((np.conj(d) * prod).real))
