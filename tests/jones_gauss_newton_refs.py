"""References of the Gauss-Newton product with 2 x 2 Jones gains and a Jones direction (``simulate_vis_jones_gauss_newton``,
``fv_sim_jones_weight_block``, ``fv_jones_weight_rows``) in numpy fp64, straight from the definitions, built on
``jones_refs`` (whose array layout this module shares: ``V``, ``w`` and the parts in ``simulate_vis``'s polarized block shape
``lead + (2, 2, nbls)``, ``J`` and ``dJ`` in ``lead + (2, 2, nant)``).  With ``G1 = J[a1]``, ``G2 = J[a2]``, ``H1 = dJ[a1]``,
``H2 = dJ[a2]``, U the sum of the parts and V the forward:

    U'[x, y]  = sum conj(G1[y', y]) G2[x', x] U[x', y']
              + sum conj(H1[y', y]) G2[x', x] V[x', y'] + sum conj(G1[y', y]) H2[x', x] V[x', y']   (with a direction)
    G'        = 2 (w U')             quad row += w |U'|^2
    stored G[x', y'] = sum conj(G2[x', x]) G'[x, y] G1[y', y]
    hjones    = ``jones_refs.chi2_jones``' gjones with this G'
"""

import numpy as np

from tests import jones_refs


def _product(X, A, B, a1, a2):
    """``sum conj(A[a1][y', y]) B[a2][x', x] X[x', y']``: ``jones_refs.apply_jones`` with two different sets of matrices."""
    return np.einsum("...bdk,...ack,...abk->...cdk", np.conj(np.asarray(A, dtype=np.complex128)[..., a1]),
                     np.asarray(B, dtype=np.complex128)[..., a2], X)


def tangent(parts, V, J, dJ, a1, a2):
    """``U'`` in fp64, U the sum of ``parts`` (an empty list: 0) and ``dJ`` None meaning no Jones direction."""
    V = np.asarray(V, dtype=np.complex128)
    U = np.zeros(V.shape, dtype=np.complex128)
    for p in parts:
        U = U + np.asarray(p, dtype=np.complex128)
    Up = _product(U, J, J, a1, a2)
    if dJ is not None:
        Up = Up + _product(V, dJ, J, a1, a2) + _product(V, J, dJ, a1, a2)
    return Up


def jones_gauss_newton(parts, V, w, J, dJ, a1, a2, with_abs=False):
    """``(rows, G', G, hjones)`` in fp64: ``rows = sum over the row of w |U'|^2``, ``G' = 2 w U'``, the stored G and
    ``hjones`` (``J``'s shape), the matrices' block of H p.  ``w`` None means 1; where ``w == 0`` that one sample is flagged:
    it adds nothing anywhere, while the baseline's other samples still use all four values of U and V; a baseline whose
    four samples are all flagged uses neither its parts nor ``V`` (they may be NaN there).  ``with_abs=True`` appends
    ``(S_tot, A)``: ``S_tot = sum |G1| |G2| |U| + sum |H1| |G2| |V| + sum |G1| |H2| |V|``, the majorant of U', and A,
    ``hjones``' formula with every factor replaced by its modulus and G' by ``2 w S_tot``."""
    V = np.asarray(V, dtype=np.complex128)
    J = np.asarray(J, dtype=np.complex128)
    a1, a2 = np.asarray(a1), np.asarray(a2)
    w = np.ones(V.shape) if w is None else np.asarray(w, dtype=np.float64)
    used = w != 0
    live = used.any(axis=(-3, -2), keepdims=True)  # baselines with a sample that counts
    V = np.where(live, V, 0)
    parts = [np.where(live, np.asarray(p, dtype=np.complex128), 0) for p in parts]
    G1, G2 = J[..., a1], J[..., a2]
    Up = np.where(used, tangent(parts, V, J, dJ, a1, a2), 0)
    rows = (w * (Up.real**2 + Up.imag**2)).reshape(V.shape[:-3] + (-1,)).sum(axis=-1)
    Gp = 2 * w * Up
    G = np.einsum("...ack,...cdk,...bdk->...abk", np.conj(G2), Gp, G1)
    hj = np.zeros(J.shape, dtype=np.complex128)
    first, second = jones_refs._sides(V, Gp, G1, G2)
    np.add.at(hj, (Ellipsis, a1), first)
    np.add.at(hj, (Ellipsis, a2), second)
    out = (rows, Gp, G, hj)
    if with_abs:
        absU = np.zeros(V.shape)
        for p in parts:
            absU = absU + np.abs(p)  # (|U| <= the sum of the parts' moduli: the parts are added in T too)
        S = _product(absU, np.abs(J), np.abs(J), a1, a2).real
        if dJ is not None:
            S = S + _product(np.abs(V), np.abs(dJ), np.abs(J), a1, a2).real + _product(np.abs(V), np.abs(J), np.abs(dJ), a1, a2).real
        A = np.zeros(J.shape)
        first, second = jones_refs._sides(np.abs(V), np.where(used, 2 * w * S, 0), np.abs(G1), np.abs(G2))
        np.add.at(A, (Ellipsis, a1), first.real)
        np.add.at(A, (Ellipsis, a2), second.real)
        out += (S, A)
    return out


def inner_jones(dJ, hjones):
    """The matrices' part of ``<p, H p>``: ``Re sum conj(dJ) hjones``."""
    return float(np.sum((np.conj(np.asarray(dJ, dtype=np.complex128)) * np.asarray(hjones)).real))
