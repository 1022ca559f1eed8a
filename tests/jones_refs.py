"""References of the Jones gains in the fused objective (``simulate_vis_jones_chi2``, ``fv_sim_run_residual_jones``,
``fv_jones_residual_chi2``) in numpy fp64, straight from the definition.

Arrays: ``V``, ``d``, ``w`` have ``simulate_vis``'s polarized block shape ``lead + (2, 2, nbls)``; the matrices ``J`` are
``lead + (2, 2, nant)``, the engine's block layout, ``J[.., i, j, a] = Gamma_a[i, j]`` with ``i`` the feed of the ideal
antenna and ``j`` the measured one; ``a1``, ``a2`` are the antenna rows of every baseline.  The polarized output
``[.., x, y, k]`` is ``(A_a1^H C A_a2)[y, x]``: its MINOR feed axis ``y`` is the first (conjugated) antenna's, so with
``A_a -> A_a Gamma_a``

    ``V'[x, y] = sum_{x', y'} conj(Gamma_a1[y', y]) Gamma_a2[x', x] V[x', y']``.

Diagonal matrices ``Gamma_a = diag(g[a])`` are ``gain_refs``' gains."""

import numpy as np

from tests.gain_refs import five_point  # noqa: F401  (the stencil the tests of both references use)


def diagonal(g):
    """The matrices ``diag(g)`` of polarized gains ``g``, ``lead + (2, nant)``."""
    g = np.asarray(g)
    J = np.zeros(g.shape[:-2] + (2, 2, g.shape[-1]), dtype=g.dtype)
    J[..., 0, 0, :] = g[..., 0, :]
    J[..., 1, 1, :] = g[..., 1, :]
    return J


def apply_jones(V, J, a1, a2):
    """``V'``, by einsum: x' = a, y' = b, x = c, y = d."""
    V = np.asarray(V, dtype=np.complex128)
    J = np.asarray(J, dtype=np.complex128)
    return np.einsum("...bdk,...ack,...abk->...cdk", np.conj(J[..., a1]), J[..., a2], V)


def _sides(V, Gp, G1, G2):
    """The per-baseline terms of the two sides of the gradient: ``first[y', y]`` belongs to ``a1``, ``second[x', x]`` to
    ``a2``.  ``G1`` enters conjugated in ``V'``: the caller passes what stands in the formulas (moduli for the majorant)."""
    M = np.einsum("...ack,...abk->...cbk", G2, V)  # (Gamma_2^T V)[x, y']
    first = np.einsum("...cdk,...cbk->...bdk", np.conj(Gp), M)
    B = np.einsum("...abk,...bdk->...adk", V, np.conj(G1))  # (V conj Gamma_1)[x', y]
    second = np.einsum("...cdk,...adk->...ack", Gp, np.conj(B))
    return first, second


def chi2_jones(V, d, w, J, a1, a2, with_abs=False):
    """``(rows, G', G, gjones)`` in fp64: ``rows = sum over the row of w |V' - d|^2``, ``G' = 2 w (V' - d)``,
    ``G[x', y'] = sum conj(Gamma_2[x', x]) G'[x, y] Gamma_1[y', y] = d chi2 / dV`` and ``gjones`` (``J``'s shape) with
    ``d chi2 = Re sum conj(gjones) dJ``.  ``w`` None means 1; where ``w == 0`` that one sample is flagged as in
    ``gain_refs.chi2_gains``: it adds nothing anywhere and ``d`` is not used (it may be NaN); the baseline's other samples
    still use all four values of ``V``.  ``with_abs=True`` appends A, ``gjones``' formula with every factor replaced by its
    modulus and ``delta`` by ``S + |d|``, ``S = sum |Gamma_1| |Gamma_2| |V|``, over the unflagged samples."""
    V = np.asarray(V, dtype=np.complex128)
    J = np.asarray(J, dtype=np.complex128)
    a1, a2 = np.asarray(a1), np.asarray(a2)
    w = np.ones(V.shape) if w is None else np.asarray(w, dtype=np.float64)
    used = w != 0
    dz = np.where(used, np.asarray(d, dtype=np.complex128), 0)
    G1, G2 = J[..., a1], J[..., a2]
    delta = np.where(used, apply_jones(V, J, a1, a2) - dz, 0)
    rows = (w * (delta.real**2 + delta.imag**2)).reshape(V.shape[:-3] + (-1,)).sum(axis=-1)
    Gp = 2 * w * delta
    G = np.einsum("...ack,...cdk,...bdk->...abk", np.conj(G2), Gp, G1)
    gj = np.zeros(J.shape, dtype=np.complex128)
    first, second = _sides(V, Gp, G1, G2)
    np.add.at(gj, (Ellipsis, a1), first)
    np.add.at(gj, (Ellipsis, a2), second)
    out = (rows, Gp, G, gj)
    if with_abs:
        S = apply_jones(np.abs(V), np.abs(J), a1, a2).real
        A = np.zeros(J.shape)
        first, second = _sides(np.abs(V), np.where(used, 2 * w * (S + np.abs(dz)), 0), np.abs(G1), np.abs(G2))
        np.add.at(A, (Ellipsis, a1), first.real)
        np.add.at(A, (Ellipsis, a2), second.real)
        out += (A,)
    return out
