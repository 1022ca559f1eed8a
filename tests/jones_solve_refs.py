"""References of the Jones solve on a resident model (``simulate_vis_jones_solve``, ``fv_jones_solve``,
``fv_jones_normal_rows``) in numpy fp64, straight from the definitions, built on ``jones_refs``.

Arrays as in ``jones_refs``: ``V``, ``d``, ``w`` have ``simulate_vis``'s polarized block shape ``lead + (2, 2, nbls)``,
``[.., x, y, k]`` with ``y`` the feed of ``a1`` (the conjugated antenna) and ``x`` of ``a2``; the matrices ``J`` are
``lead + (2, 2, nant)``, ``J[.., i, j, a] = Gamma_a[i, j]``.  A sample is used when ``w > 0`` and ``a1 != a2``
(auto-correlations count as flagged); a flagged datum is not used and may be NaN.  With ``G1 = Gamma[a1]``,
``G2 = Gamma[a2]``, per antenna ``a`` and column ``c`` of ``Gamma_a``:

    side 1 (a = a2, c = x), ``Z[x', y] = sum_{y'} V[x', y'] conj(G1[y', y])``:
        ``A[i, j] += w[x, y] conj(Z[i, y]) Z[j, y]``,   ``b[i] += w[x, y] conj(Z[i, y]) d[x, y]``,   summed over y;
    side 0 (a = a1, c = y), ``Y[x, y'] = sum_{x'} G2[x', x] V[x', y']``:
        ``A[i, j] += w[x, y] Y[x, i] conj(Y[x, j])``,   ``b[i] += w[x, y] Y[x, i] conj(d[x, y])``,   summed over x.

``A`` is held as ``lead + (4, 2, nant)`` float64 = [A00, A11, Re A01, Im A01] x column x antenna, ``b`` as
``lead + (2, 2, nant)`` complex128 ``[i, column, a]``, and ``gjones[:, c, a] = 2 (A Gamma_a[:, c] - b)`` with the autos
flagged."""

import numpy as np

from tests import jones_refs
from tests.gain_solve_refs import used_weights

RANK = 2.0**-30  # a column is solved when A00 > 0, A11 > 0 and det > RANK A00 A11


def _full(A):
    """The Hermitian matrices ``lead + (2 (i), 2 (j), 2 (column), nant)`` of the packed ``A``."""
    a01 = A[..., 2, :, :] + 1j * A[..., 3, :, :]
    return np.stack([np.stack([A[..., 0, :, :] + 0j, a01], axis=-3), np.stack([np.conj(a01), A[..., 1, :, :] + 0j], axis=-3)], axis=-4)


def normal_sums(V, d, w, J, a1, a2, with_abs=False):
    """``(A, b)``, packed as the module docstring says.  ``with_abs=True`` appends the majorants ``(A_abs, b_abs)`` in the
    same layouts (``b_abs`` float64), with every factor replaced by its modulus."""
    J = np.asarray(J, dtype=np.complex128)
    a1, a2 = np.asarray(a1), np.asarray(a2)
    w = used_weights(V, w, a1, a2)
    used = w > 0
    V = np.asarray(V, dtype=np.complex128)
    d = np.where(used, np.asarray(d, dtype=np.complex128), 0)

    def sums(V, d, G1c, G2, conj):
        """``G1c`` stands where ``conj(G1)`` stands in the formulas; ``conj`` conjugates (the identity for the moduli)."""
        lead = J.shape[:-3]
        nant = J.shape[-1]
        Z = np.einsum("...abk,...bdk->...adk", V, G1c)  # Z[x', y]
        Y = np.einsum("...ack,...abk->...cbk", G2, V)  # Y[x, y']
        # side 1, antenna a2, column x: per baseline [i, j, x] and [i, x]
        A1 = np.einsum("...xyk,...iyk,...jyk->...ijxk", w, conj(Z), Z)
        b1 = np.einsum("...xyk,...iyk,...xyk->...ixk", w, conj(Z), d)
        # side 0, antenna a1, column y: per baseline [i, j, y] and [i, y]
        A0 = np.einsum("...xyk,...xik,...xjk->...ijyk", w, Y, conj(Y))
        b0 = np.einsum("...xyk,...xik,...xyk->...iyk", w, Y, conj(d))
        Af = np.zeros(lead + (2, 2, 2, nant), dtype=np.complex128)
        b = np.zeros(lead + (2, 2, nant), dtype=np.complex128)
        np.add.at(Af, (Ellipsis, a2), A1)
        np.add.at(Af, (Ellipsis, a1), A0)
        np.add.at(b, (Ellipsis, a2), b1)
        np.add.at(b, (Ellipsis, a1), b0)
        A = np.stack([Af[..., 0, 0, :, :].real, Af[..., 1, 1, :, :].real, Af[..., 0, 1, :, :].real, Af[..., 0, 1, :, :].imag], axis=-3)
        return A, b

    # (a baseline without a used sample adds exact zeros: w is 0 there)
    out = sums(V, d, np.conj(J[..., a1]), J[..., a2], np.conj)
    if with_abs:
        A_abs, b_abs = sums(np.abs(V), np.abs(d), np.abs(J[..., a1]), np.abs(J[..., a2]), lambda x: x)
        A_abs[..., 3, :, :] = A_abs[..., 2, :, :]  # (the majorant of either part of A01)
        out += (A_abs, b_abs.real)
    return out


def gradient(A, b, J):
    """``2 (A Gamma[:, c] - b)`` in ``J``'s layout."""
    return 2 * (np.einsum("...ijca,...jca->...ica", _full(A), J) - b)


def chi2_rows(V, d, w, J, a1, a2):
    """``sum w |V' - d|^2`` over the used samples per row of ``lead``: ``jones_refs.chi2_jones`` with the autos zeroed."""
    return jones_refs.chi2_jones(V, d, used_weights(V, w, a1, a2), J, a1, a2)[0]


def solve_columns(A, b, J):
    """``(hat, solved)``: ``A^-1 b`` by the closed form where the rank rule holds (else ``J``'s own entries), in ``J``'s
    layout, and the bool array ``lead + (2, nant)`` per column and antenna."""
    a00, a11, a01 = A[..., 0, :, :], A[..., 1, :, :], A[..., 2, :, :] + 1j * A[..., 3, :, :]
    det = a00 * a11 - (a01.real**2 + a01.imag**2)
    solved = (a00 > 0) & (a11 > 0) & (det > RANK * (a00 * a11))
    safe = np.where(solved, det, 1.0)
    b0, b1 = b[..., 0, :, :], b[..., 1, :, :]
    hat = np.stack([(a11 * b0 - a01 * b1) / safe, (a00 * b1 - np.conj(a01) * b0) / safe], axis=-3)
    return np.where(solved[..., None, :, :], hat, J), solved


def solve(V, d, w, J0, a1, a2, per_time, max_iter, tol):
    """The alternating per-antenna solve on ``(nfreqs, ntimes, 2, 2, nbls)`` blocks.  ``J0``: the start,
    ``(nfreqs, ntimes if per_time else 1, 2, 2, nant)``.  Iteration i = 1, 2, ...: the normal systems at the current
    matrices (time-constant: added over the times in ascending order), the columns' solutions under the rank rule,
    ``Gamma <- Gamma^`` for odd i and ``(Gamma^ + Gamma) / 2`` for even i; per unit ``change = max |new - old| / max |new|``;
    the loop ends after the first iteration at which every unit has ``change < tol``, or at ``max_iter``.  Returns
    ``(matrices, changes, chi2, solved, (A, b))``: ``J0``'s shape, the list of every iteration's per-unit change, the
    ``(nfreqs, ntimes)`` chi2 at the returned matrices, the bool array ``J0.shape[:2] + (2, nant)`` and the summed systems
    of the last iteration."""
    J = np.array(J0, dtype=np.complex128)
    nt = np.shape(V)[1]
    changes, solved, last = [], np.zeros(J.shape[:2] + J.shape[3:], dtype=bool), None

    def per_row(x):
        return x if per_time else np.broadcast_to(x, (x.shape[0], nt) + x.shape[2:])

    for i in range(1, max_iter + 1):
        A, b = normal_sums(V, d, w, per_row(J), a1, a2)
        if not per_time:
            tA, tb = np.zeros(A[:, :1].shape), np.zeros(b[:, :1].shape, dtype=np.complex128)
            for t in range(nt):
                tA[:, 0] += A[:, t]
                tb[:, 0] += b[:, t]
            A, b = tA, tb
        last = (A, b)
        hat, solved = solve_columns(A, b, J)
        new = np.where(solved[..., None, :, :], hat if i % 2 else 0.5 * (hat + J), J)
        top = np.abs(new).max(axis=(2, 3, 4))
        changes.append(np.where(top > 0, np.abs(new - J).max(axis=(2, 3, 4)) / np.where(top > 0, top, 1.0), 0.0))
        J = new
        if np.all(changes[-1] < tol):
            break
    return J, changes, chi2_rows(V, d, w, per_row(J), a1, a2), solved, last
