"""References of redundant calibration (``redundant_gain_solve``, ``fv_redundant_solve``, ``fv_redundant_vis_rows``,
``fv_redundant_normal_rows``) in numpy fp64, straight from the definitions, built on ``gain_refs`` and ``gain_solve_refs``.

Arrays as there: ``d``, ``w`` have ``simulate_vis``'s block shape ``lead + (nbls,)`` or ``lead + (2, 2, nbls)``; the gains are
``lead + (nfeed, nant)``; the group visibilities ``U`` are ``lead + (ngroups,)`` or ``lead + (2, 2, ngroups)`` and
``group[k]`` is the group of baseline k, so that the model of the block is ``U[..., group]``.  A sample is used when
``w > 0`` and ``a1 != a2``; a flagged sample is not used and may be NaN."""

import numpy as np

from tests import gain_refs
from tests import gain_solve_refs as gsr


def _group_sums(x, group, ngroups):
    out = np.zeros(x.shape[:-1] + (ngroups,), dtype=x.dtype)
    np.add.at(out, (Ellipsis, np.asarray(group)), x)
    return out


def vis_step(d, w, g, a1, a2, group, ngroups, U0=None, with_abs=False):
    """The U-step: with ``m = conj(g[p, a1]) g[q, a2]``, per (lead, pol, group) over the group's used samples
    ``num = sum w conj(m) d``, ``den = sum w |m|^2`` and ``U = num / den`` where ``den > 0``, else ``U0`` (None: 0).  Returns
    ``(U, den)``; ``with_abs=True`` appends the sums of the moduli of ``num``'s terms."""
    g = np.asarray(g, dtype=np.complex128)
    pol = gain_refs._polarized(d, g)
    w = gsr.used_weights(d, w, a1, a2)
    used = w > 0
    d = np.where(used, np.asarray(d, dtype=np.complex128), 0)
    m = gain_refs.gain_product(g, np.asarray(a1), np.asarray(a2), pol)
    terms = w * (np.conj(m) * d)
    num = _group_sums(terms, group, ngroups)
    den = _group_sums(w * (m.real**2 + m.imag**2), group, ngroups)
    U = np.zeros(num.shape, dtype=np.complex128) if U0 is None else np.array(U0, dtype=np.complex128)
    ok = den > 0
    safe = np.where(ok, den, 1.0)
    U[ok] = (num.real / safe + 1j * (num.imag / safe))[ok]
    out = (U, den)
    if with_abs:
        out += (_group_sums(np.abs(terms), group, ngroups),)
    return out


def model(U, group):
    """The block's model: every baseline's group visibility."""
    return np.asarray(U)[..., np.asarray(group)]


def normal_sums(U, d, w, g, a1, a2, group, with_abs=False):
    """``gain_solve_refs.normal_sums`` with ``V = U[..., group]``."""
    return gsr.normal_sums(model(U, group), d, w, g, a1, a2, with_abs=with_abs)


def chi2_rows(U, d, w, g, a1, a2, group):
    """``sum w |conj(g[a1]) g[a2] U[group] - d|^2`` over the used samples per row of ``lead``."""
    return gsr.chi2_rows(model(U, group), d, w, g, a1, a2)


def solve(d, w, g0, a1, a2, group, ngroups, per_time, max_iter, tol):
    """The alternating solve on ``(nfreqs, ntimes, ...)`` blocks.  ``g0``: ``(nfreqs, ntimes if per_time else 1, nfeed,
    nant)``; U starts from 0 and is per row.  Iteration i = 1, 2, ...: the U-step at the current gains; the normal sums at
    these U (time-constant: added over the times in ascending order), ``g^ = num / den`` where ``den > 0``, ``g <- g^`` for
    odd i and ``(g^ + g) / 2`` for even i; per unit ``change = max |g_new - g| / max |g_new|``; the loop ends after the first
    iteration at which every unit has ``change < tol``, or at ``max_iter``.  Then one more U-step at the returned gains.
    Returns ``(gains, U, changes, chi2, solved, vis_solved)``."""
    g = np.array(g0, dtype=np.complex128)
    nt = np.shape(d)[1]
    changes, solved, U = [], np.zeros(g.shape, dtype=bool), None

    def per_row(x):
        return x if per_time else np.broadcast_to(x, (x.shape[0], nt) + x.shape[2:])

    for i in range(1, max_iter + 1):
        U, _ = vis_step(d, w, per_row(g), a1, a2, group, ngroups, U)
        num, den = normal_sums(U, d, w, per_row(g), a1, a2, group)
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
    U, den = vis_step(d, w, per_row(g), a1, a2, group, ngroups, U)
    return g, U, changes, chi2_rows(U, d, w, per_row(g), a1, a2, group), solved, den > 0
