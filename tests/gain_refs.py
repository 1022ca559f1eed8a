"""References of the per-antenna gains in the fused objective (``simulate_vis_gain_chi2``, ``fv_sim_run_residual_gains``,
``fv_gain_residual_chi2``) in numpy fp64, straight from the definition.

Arrays: ``V``, ``d``, ``w`` have ``simulate_vis``'s block shape ``lead + (nbls,)`` (unpolarized) or ``lead + (2, 2, nbls)``
(polarized); the gains ``g`` are ``lead + (nfeed, nant)``, the engine's block layout; ``a1``, ``a2`` are the antenna rows of
every baseline.  The polarized output ``[.., x, y, k]`` is ``(A_a1^H C A_a2)[y, x]``: its MINOR feed axis ``y`` is the first
(conjugated) antenna's, so ``m[.., x, y, k] = conj(g[.., y, a1[k]]) g[.., x, a2[k]]``."""

import numpy as np


def _polarized(V, g):
    return np.ndim(V) == np.ndim(g) + 1


def gain_product(g, a1, a2, polarized):
    """``m``, in ``V``'s shape."""
    g = np.asarray(g, dtype=np.complex128)
    if not polarized:
        return np.conj(g[..., 0, a1]) * g[..., 0, a2]
    return g[..., :, a2][..., :, None, :] * np.conj(g[..., :, a1])[..., None, :, :]


def apply_gains(V, g, a1, a2):
    """``V' = conj(g[a1]) g[a2] V``."""
    V = np.asarray(V, dtype=np.complex128)
    return gain_product(g, a1, a2, _polarized(V, g)) * V


def _to_antennas(first, second, g_shape, a1, a2, polarized):
    """Adds the per-sample terms of the two sides to their antennas: ``first`` belongs to ``a1`` (feed ``y``), ``second``
    to ``a2`` (feed ``x``)."""
    out = np.zeros(g_shape, dtype=first.dtype)
    if not polarized:
        np.add.at(out[..., 0, :], (Ellipsis, a1), first)
        np.add.at(out[..., 0, :], (Ellipsis, a2), second)
        return out
    for x in range(2):
        for y in range(2):
            np.add.at(out[..., y, :], (Ellipsis, a1), first[..., x, y, :])
            np.add.at(out[..., x, :], (Ellipsis, a2), second[..., x, y, :])
    return out


def chi2_gains(V, d, w, g, a1, a2, with_abs=False):
    """``(rows, G', G, ggains)`` in fp64: ``rows = sum over the row of w |V' - d|^2``, ``G' = 2 w (V' - d)``,
    ``G = conj(m) G' = d chi2 / dV`` and ``ggains`` (``g``'s shape) with ``d chi2 = Re sum conj(ggains) dg``.  ``w`` None
    means 1; where ``w == 0`` the sample is flagged as in ``objective_refs.chi2_and_gvis``: it adds nothing anywhere and
    ``d`` is not used (it may be NaN).  ``with_abs=True`` appends the per-antenna sums of the moduli of ``ggains``' terms."""
    V = np.asarray(V, dtype=np.complex128)
    g = np.asarray(g, dtype=np.complex128)
    a1, a2 = np.asarray(a1), np.asarray(a2)
    pol = _polarized(V, g)
    w = np.ones(V.shape) if w is None else np.asarray(w, dtype=np.float64)
    used = w != 0
    m = gain_product(g, a1, a2, pol)
    delta = np.where(used, m * V - np.where(used, np.asarray(d, dtype=np.complex128), 0), 0)
    terms = w * (delta.real**2 + delta.imag**2)
    lead = V.ndim - (3 if pol else 1)
    rows = terms.reshape(V.shape[:lead] + (-1,)).sum(axis=-1)
    Gp = 2 * w * delta
    if pol:
        g_a2, g_a1 = g[..., :, a2][..., :, None, :], g[..., :, a1][..., None, :, :]
    else:
        g_a2, g_a1 = g[..., 0, a2], g[..., 0, a1]
    first = np.conj(Gp) * g_a2 * V  # d / d conj(g[a1]) side
    second = Gp * g_a1 * np.conj(V)
    out = (rows, Gp, np.conj(m) * Gp, _to_antennas(first, second, g.shape, a1, a2, pol))
    if with_abs:
        out += (_to_antennas(np.abs(first), np.abs(second), g.shape, a1, a2, pol),)
    return out


def five_point(f, h):
    """The five-point central stencil of ``f`` at 0 with step ``h`` (exact for a quartic up to rounding)."""
    return (f(-2 * h) - 8 * f(-h) + 8 * f(h) - f(2 * h)) / (12 * h)
