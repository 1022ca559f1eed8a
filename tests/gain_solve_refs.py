"""References of the gain solve on a resident model (``simulate_vis_gain_solve``, ``fv_gain_solve``,
``fv_gain_normal_rows``) in numpy fp64, straight from the definitions, built on ``gain_refs``.

Arrays as in ``gain_refs``: ``V``, ``d``, ``w`` have ``simulate_vis``'s block shape ``lead + (nbls,)`` or
``lead + (2, 2, nbls)``; the gains are ``lead + (nfeed, nant)``.  A sample is used when ``w > 0`` and ``a1 != a2``
(auto-correlations count as flagged); a flagged sample is not used and may be NaN."""

import numpy as np

from tests import gain_refs
from tests.gain_refs import _polarized, _to_antennas


def used_weights(V, w, a1, a2):
    """``w`` (None: ones) in ``V``'s shape as float64, with the auto-correlations zeroed."""
    w = np.ones(np.shape(V)) if w is None else np.array(w, dtype=np.float64)
    w = np.broadcast_to(w, np.shape(V)).copy()
    w[..., np.asarray(a1) == np.asarray(a2)] = 0
    return w


def normal_sums(V, d, w, g, a1, a2, with_abs=False):
    """``(num, den)`` in ``g``'s shape, complex128 and float64:
        side 0 (a = a1, feed p, every q):  num += w g[q, a2] V conj(d),   den += w |g[q, a2]|^2 |V|^2
        side 1 (a = a2, feed q, every p):  num += w g[p, a1] conj(V) d,   den += w |g[p, a1]|^2 |V|^2
    over the used samples.  ``with_abs=True`` appends the per-antenna sums of the moduli of ``num``'s terms (``den``'s terms
    are their own moduli)."""
    g = np.asarray(g, dtype=np.complex128)
    a1, a2 = np.asarray(a1), np.asarray(a2)
    pol = _polarized(V, g)
    w = used_weights(V, w, a1, a2)
    used = w > 0
    V = np.where(used, np.asarray(V, dtype=np.complex128), 0)
    d = np.where(used, np.asarray(d, dtype=np.complex128), 0)
    if pol:
        g_a2, g_a1 = g[..., :, a2][..., :, None, :], g[..., :, a1][..., None, :, :]
    else:
        g_a2, g_a1 = g[..., 0, a2], g[..., 0, a1]
    first = w * (g_a2 * V * np.conj(d))  # antenna a1's, feed y
    second = w * (g_a1 * np.conj(V) * d)  # antenna a2's, feed x
    v2 = V.real**2 + V.imag**2
    den1 = w * ((g_a2.real**2 + g_a2.imag**2) * v2)
    den2 = w * ((g_a1.real**2 + g_a1.imag**2) * v2)
    out = (_to_antennas(first, second, g.shape, a1, a2, pol), _to_antennas(den1, den2, g.shape, a1, a2, pol))
    if with_abs:
        out += (_to_antennas(np.abs(first), np.abs(second), g.shape, a1, a2, pol),)
    return out


def chi2_rows(V, d, w, g, a1, a2):
    """``sum w |V' - d|^2`` over the used samples per row of ``lead``: ``gain_refs.chi2_gains`` with the autos zeroed."""
    w = used_weights(V, w, a1, a2)
    return gain_refs.chi2_gains(np.where(w > 0, V, 0), d, w, g, a1, a2)[0]


def solve(V, d, w, g0, a1, a2, per_time, max_iter, tol):
    """The alternating per-antenna solve on ``(nfreqs, ntimes, ...)`` blocks.  ``g0``: the start,
    ``(nfreqs, ntimes if per_time else 1, nfeed, nant)``.  Iteration i = 1, 2, ...: the normal sums at the current gains
    (time-constant: added over the times in ascending order), ``g^ = num / den`` where ``den > 0`` (else the antenna keeps its
    value), ``g <- g^`` for odd i and ``(g^ + g) / 2`` for even i; per unit ``change = max |g_new - g| / max |g_new|``; the loop
    ends after the first iteration at which every unit has ``change < tol``, or at ``max_iter``.  Returns ``(gains, changes,
    chi2, solved)``: the gains in ``g0``'s shape, the list of every iteration's per-unit change (``g0.shape[:2]``), the
    ``(nfreqs, ntimes)`` chi2 at the returned gains and the bool array of ``den > 0`` at the last iteration."""
    g = np.array(g0, dtype=np.complex128)
    nt = np.shape(V)[1]
    changes, solved = [], np.zeros(g.shape, dtype=bool)

    def per_row(x):
        return x if per_time else np.broadcast_to(x, (x.shape[0], nt) + x.shape[2:])

    for i in range(1, max_iter + 1):
        num, den = normal_sums(V, d, w, per_row(g), a1, a2)
        if not per_time:
            tn, td = np.zeros(g.shape, dtype=np.complex128), np.zeros(g.shape)
            for t in range(nt):
                tn[:, 0] += num[:, t]
                td[:, 0] += den[:, t]
            num, den = tn, td
        solved = den > 0
        hat = np.where(solved, num / np.where(solved, den, 1.0), g)
        new = np.where(solved, hat if i % 2 else 0.5 * (hat + g), g)
        top = np.abs(new).max(axis=(2, 3))
        changes.append(np.where(top > 0, np.abs(new - g).max(axis=(2, 3)) / np.where(top > 0, top, 1.0), 0.0))
        g = new
        if np.all(changes[-1] < tol):
            break
    return g, changes, chi2_rows(V, d, w, per_row(g), a1, a2), solved
