"""References of the Gauss-Newton product with per-antenna gains and a gain direction (``simulate_vis_gain_gauss_newton``,
``fv_sim_gain_weight_block``, ``fv_gain_weight_rows``) in numpy fp64, straight from the definitions, built on ``gain_refs``
(whose array layout this module shares: ``V``, ``w`` and the parts in ``simulate_vis``'s block shape, ``g`` and ``dg`` in
``lead + (nfeed, nant)``).

    m  = conj(g1) g2                     dm = conj(h1) g2 + conj(g1) h2      (dm = 0 without a gain direction)
    U' = m U + dm V                      (the tangent of V' along p = (sky directions, dg))
    G' = 2 (w U')                        quad row += w |U'|^2
    stored G = conj(m) G'
    hgains[a, f] = sum_{k: a1=a, p=f} conj(G') g2 V  +  sum_{k: a2=a, q=f} G' g1 conj(V)
"""

import numpy as np

from tests import gain_refs


def tangent(parts, V, g, dg, a1, a2):
    """``U' = m U + dm V`` in fp64, U the sum of ``parts`` (an empty list: 0) and ``dg`` None meaning no gain direction."""
    V = np.asarray(V, dtype=np.complex128)
    pol = gain_refs._polarized(V, g)
    U = np.zeros(V.shape, dtype=np.complex128)
    for p in parts:
        U = U + np.asarray(p, dtype=np.complex128)
    Up = gain_refs.gain_product(g, a1, a2, pol) * U
    if dg is not None:
        h1g2 = _one_sided(dg, g, a1, a2, pol)
        g1h2 = _one_sided(g, dg, a1, a2, pol)
        Up = Up + (h1g2 + g1h2) * V
    return Up


def _one_sided(first, second, a1, a2, polarized):
    """``conj(first[a1]) second[a2]`` in ``V``'s shape."""
    first, second = np.asarray(first, dtype=np.complex128), np.asarray(second, dtype=np.complex128)
    if not polarized:
        return np.conj(first[..., 0, a1]) * second[..., 0, a2]
    return second[..., :, a2][..., :, None, :] * np.conj(first[..., :, a1])[..., None, :, :]


def gain_gauss_newton(parts, V, w, g, dg, a1, a2, with_abs=False):
    """``(rows, G', G, hgains)`` in fp64: ``rows = sum over the row of w |U'|^2``, ``G' = 2 w U'``, ``G = conj(m) G'`` and
    ``hgains`` (``g``'s shape), the gain block of H p.  ``w`` None means 1; where ``w == 0`` the sample is flagged: it adds
    nothing anywhere and neither the parts nor ``V`` are used there (they may be NaN).  ``with_abs=True`` appends the
    per-antenna sums of the moduli of ``hgains``' terms."""
    V = np.asarray(V, dtype=np.complex128)
    g = np.asarray(g, dtype=np.complex128)
    a1, a2 = np.asarray(a1), np.asarray(a2)
    pol = gain_refs._polarized(V, g)
    w = np.ones(V.shape) if w is None else np.asarray(w, dtype=np.float64)
    used = w != 0
    V = np.where(used, V, 0)
    parts = [np.where(used, np.asarray(p, dtype=np.complex128), 0) for p in parts]
    m = gain_refs.gain_product(g, a1, a2, pol)
    Up = np.where(used, tangent(parts, V, g, dg, a1, a2), 0)
    terms = w * (Up.real**2 + Up.imag**2)
    lead = V.ndim - (3 if pol else 1)
    rows = terms.reshape(V.shape[:lead] + (-1,)).sum(axis=-1)
    Gp = 2 * w * Up
    if pol:
        g_a2, g_a1 = g[..., :, a2][..., :, None, :], g[..., :, a1][..., None, :, :]
    else:
        g_a2, g_a1 = g[..., 0, a2], g[..., 0, a1]
    first = np.conj(Gp) * g_a2 * V
    second = Gp * g_a1 * np.conj(V)
    out = (rows, Gp, np.conj(m) * Gp, gain_refs._to_antennas(first, second, g.shape, a1, a2, pol))
    if with_abs:
        out += (gain_refs._to_antennas(np.abs(first), np.abs(second), g.shape, a1, a2, pol),)
    return out


def inner_gains(dg, hgains):
    """The gains' part of ``<p, H p>``: ``Re sum conj(dg) hgains``."""
    return float(np.sum((np.conj(np.asarray(dg, dtype=np.complex128)) * np.asarray(hgains)).real))
