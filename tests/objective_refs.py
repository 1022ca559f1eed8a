"""References of the fused objective (``simulate_vis_chi2``, ``fv_sim_run_residual``, ``fv_residual_chi2``) in numpy fp64."""

import math

import numpy as np


def chi2_and_gvis(V, d, w=None):
    """(chi2_rows, G) in fp64 for a block whose rows are the leading two axes (frequency, time) -- or, for a 2-D block,
    the leading one: ``chi2_rows = sum over the row of w |V - d|^2`` and ``G = 2 w (V - d)``.  ``w`` None means 1; where
    ``w == 0`` the sample is flagged: it adds 0, G is 0 and ``d`` is not used (it may be NaN)."""
    V = np.asarray(V, dtype=np.complex128)
    w = np.ones(V.shape) if w is None else np.asarray(w, dtype=np.float64)
    used = w != 0
    delta = np.where(used, V - np.where(used, np.asarray(d, dtype=np.complex128), 0), 0)
    lead = 1 if V.ndim == 2 else 2
    terms = w * (delta.real**2 + delta.imag**2)
    return terms.reshape(V.shape[:lead] + (-1,)).sum(axis=-1), 2 * w * delta


def row_sums_exact(terms):
    """``math.fsum`` of every row of a 2-D array of fp64 terms: the correctly rounded sums."""
    return np.array([math.fsum(row) for row in np.asarray(terms, dtype=np.float64)])


def row_major_sum(chi2_ft):
    """The entries of ``chi2_ft`` added one after the other in row-major order, as ``chi2_per="total"`` adds them."""
    s = 0.0
    for x in np.asarray(chi2_ft, dtype=np.float64).ravel():
        s = s + float(x)
    return s
