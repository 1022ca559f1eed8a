"""References of firstcal (``redundant_firstcal``, ``fv_firstcal_pair_delays``, ``fv_firstcal_offsets``) in numpy, straight from
the definitions and built on ``redundant_refs``.  The pair-delay stage takes a ``dtype``: ``np.float64`` is the reference,
``np.longdouble`` the variant it is checked against.

Arrays as in ``redundant_refs``: ``d``, ``w`` are ``(nfreqs, ntimes, nbls)`` or ``(nfreqs, ntimes, 2, 2, nbls)`` blocks, a sample is
used when ``w > 0`` and ``a1 != a2``, a flagged sample may be NaN.  Per-antenna quantities of this module are ``(nfeed, nant)``
and per-pair ones ``(nfeed, npairs)``.

The rounding bound of the refined bin x (``x_bound``).  P(x) = sum_f z[f] exp(-2 pi i x f / ND) is a sum of nfreqs terms whose
phases come from t = x f / ND, |t| <= nfreqs / 2 turns, formed with two roundings: a phase error of at most 2 pi * 2 u *
nfreqs / 2 = pi nfreqs eps (u = eps / 2); the sine and cosine, the complex product and the sum add a few eps and
log2(nfreqs) eps more.  So |dP| <= (pi nfreqs + 16) eps S per implementation, S = sum_f |z[f]|, and with |P| <= S the power
y = |P|^2 of two implementations differs by at most  e = 2 * 2 * (pi nfreqs + 16) eps S^2 <= C (nfreqs + 4) eps S^2, C = 16.
(S^2 in place of y: at a noiseless peak they are equal, and a point far from the peak has an error that its own small y does
not bound.)  A round's step is s = 0.5 h (y- - y+) / den, den = y- - 2 y0 + y+, |s| <= h after the clip:
    |ds| <= 0.5 h (2 e / |den| + |y- - y+| 4 e / den^2) = h e / |den| + 4 |s| e / |den| <= 5 h e / |den|.
The rounds are added up: a shift of a round's centre moves x + s by less than that shift (for an exact parabola not at all), so
the bound of x after four rounds is  sum_r 5 h_r e / |den_r|.  Where den is within 3 e of 0 the rule ``den < 0`` itself may go
either way and the bound is infinite."""

import numpy as np

from tests import gain_solve_refs as gsr
from tests import redundant_refs as rr

C_BOUND = 16.0
ROUNDS = (1.0, 0.25, 0.0625, 0.015625)


def pairs(group):
    """Consecutive members of every group, members in ascending baseline index: ``(pair1, pair2)``, int32."""
    group = np.asarray(group)
    p1, p2 = [], []
    for r in np.unique(group):
        mem = np.flatnonzero(group == r)
        p1 += list(mem[:-1])
        p2 += list(mem[1:])
    return np.array(p1, dtype=np.int32), np.array(p2, dtype=np.int32)


def _cdtype(dtype):
    return np.clongdouble if dtype == np.longdouble else np.complex128


def products(d, w, a1, a2, pair1, pair2, dtype=np.float64):
    """``z[feed, pair, f] = sum_t d[k] conj(d[k'])`` over the times at which both samples are used, times ascending; feed p of
    a polarized block reads ``[p, p]``.  Returns ``(z, z_abs)``, the second the sums of the terms' moduli."""
    used = gsr.used_weights(d, w, a1, a2) > 0
    dd = np.where(used, d, 0).astype(_cdtype(dtype))
    hands = [(dd, used)] if dd.ndim == 3 else [(dd[:, :, p, p], used[:, :, p, p]) for p in range(2)]
    nf, nt = dd.shape[:2]
    z = np.zeros((len(hands), len(pair1), nf), dtype=_cdtype(dtype))
    z_abs = np.zeros(z.shape, dtype=dtype)
    for p, (x, ok) in enumerate(hands):
        for t in range(nt):
            both = ok[:, t][:, pair1] & ok[:, t][:, pair2]
            term = np.where(both, x[:, t][:, pair1] * np.conj(x[:, t][:, pair2]), 0)
            z[p] += term.T
            z_abs[p] += np.abs(term).T
    return z, z_abs


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def periodogram(z, pad, dtype=np.float64):
    """``|P[n]|^2``, ``P[n] = sum_f z[f] tw[(n f) mod ND]``, ``tw[j] = exp(-2 pi i j / ND)``: ``(..., ND)``."""
    nf = z.shape[-1]
    nd = pad * nf
    tw = np.exp(-2j * _pi(dtype) * np.arange(nd).astype(dtype) / nd).astype(_cdtype(dtype))
    idx = (np.arange(nd)[:, None] * np.arange(nf)[None, :]) % nd
    P = z.astype(_cdtype(dtype)) @ tw[idx].T
    return P.real**2 + P.imag**2


def power_at(z, x, pad, dtype=np.float64):
    """``|P(x)|^2`` at the continuous bins ``x`` (one per row of ``z``)."""
    nf = z.shape[-1]
    t = np.asarray(x, dtype=dtype)[..., None] * np.arange(nf).astype(dtype) / dtype(pad * nf)
    t = t - np.round(t)  # (exact: the turns are dropped before the exponential)
    P = (z.astype(_cdtype(dtype)) * np.exp(-2j * _pi(dtype) * t)).sum(axis=-1)
    return P.real**2 + P.imag**2


def pair_delays(z, pad, dtype=np.float64, peak=None):
    """The coarse peak and its refinement for every row of ``z`` ``(..., nfreqs)``.  Returns a dict: ``peak_bin`` (signed),
    ``x`` (bins), ``power``, ``total``, ``used``, ``x_bound`` (the rounding bound of x, see the module's docstring), ``y`` (the
    coarse periodogram) and ``e`` (the bound of one power).  ``peak``: signed bins to refine from in place of the coarse
    peak (another implementation's, where two bins are equal within ``e``)."""
    z = np.asarray(z)
    nf = z.shape[-1]
    nd = pad * nf
    eps = np.finfo(np.float64).eps
    used = (z != 0).sum(axis=-1) >= 2
    total = (z.real**2 + z.imag**2).sum(axis=-1).astype(np.float64)
    e = (C_BOUND * (nf + 4) * eps * np.abs(z).sum(axis=-1) ** 2).astype(np.float64)
    y = periodogram(z, pad, dtype)
    n = np.argmax(y, axis=-1)  # (the lowest n of maximal power)
    peak = np.where(2 * n >= nd, n - nd, n) if peak is None else np.asarray(peak)
    x = peak.astype(dtype)
    bound = np.zeros(x.shape)
    for h in ROUNDS:
        ym, y0, yp = (power_at(z, x + s * dtype(h), pad, dtype) for s in (-1, 0, 1))
        den = ym - 2 * y0 + yp
        ok = den < 0
        step = np.clip(dtype(0.5 * h) * (ym - yp) / np.where(ok, den, 1), -h, h)
        x = np.where(ok, x + step, x)
        with np.errstate(divide="ignore", invalid="ignore"):
            bound += np.where(np.abs(den) > 3 * e, 5 * h * e / np.abs(den).astype(np.float64), np.inf)
    power = power_at(z, x, pad, dtype)
    zero = ~used
    return dict(peak_bin=np.where(zero, 0, peak).astype(np.int32), x=np.where(zero, 0, x), power=np.where(zero, 0, power), total=total,
                used=used, x_bound=np.where(zero, 0.0, bound), y=y, e=e)


def pair_matrix(a1, a2, pair1, pair2, nant):
    """``A tau = dtau``: row r has +1 at a2[k] and a1[k'], -1 at a1[k] and a2[k']."""
    A = np.zeros((len(pair1), nant))
    r = np.arange(len(pair1))
    for col, sign in ((a2[pair1], 1.0), (a1[pair2], 1.0), (a1[pair1], -1.0), (a2[pair2], -1.0)):
        np.add.at(A, (r, col), sign)
    return A


def antenna_delays(x, used, x_bound, A, nd, dnu):
    """The minimum-norm least-squares antenna delays of the used pairs, per feed, in seconds, with the pairs' bounds
    propagated through the pseudo-inverse: ``(tau, tau_bound, in_pair)``, each ``(nfeed, nant)``."""
    nfeed, nant = x.shape[0], A.shape[1]
    tau, bound, in_pair = np.zeros((nfeed, nant)), np.zeros((nfeed, nant)), np.zeros((nfeed, nant), dtype=bool)
    for p in range(nfeed):
        rows = np.asarray(used[p], dtype=bool)
        if not rows.any():
            continue
        tau[p] = np.linalg.lstsq(A[rows], np.asarray(x[p], dtype=np.float64)[rows] / (nd * dnu), rcond=None)[0]
        bound[p] = np.abs(np.linalg.pinv(A[rows])) @ (np.asarray(x_bound[p])[rows] / abs(nd * dnu))
        in_pair[p] = np.abs(A[rows]).sum(axis=0) > 0
    tau[~in_pair] = 0
    return tau, bound, in_pair


def derotate(d, a1, a2, slopes):
    """``d'[f, t, pol, k] = d exp(-i (f - (nfreqs - 1) / 2) (s[q, a2] - s[p, a1]))``, ``p = pol & 1``, ``q = pol >> 1``
    (the block's ``[q, p]``)."""
    nf = d.shape[0]
    c = np.arange(nf) - 0.5 * (nf - 1)
    lead = (nf,) + (1,) * (d.ndim - 1)
    if d.ndim == 3:
        return d * np.exp(-1j * c.reshape(lead) * (slopes[0, a2] - slopes[0, a1]))
    out = np.array(d, dtype=np.complex128)
    for q in range(2):
        for p in range(2):
            out[:, :, q, p] = d[:, :, q, p] * np.exp(-1j * c.reshape(nf, 1, 1) * (slopes[q, a2] - slopes[p, a1]))
    return out


def offsets(d, w, a1, a2, group, ngroups, slopes, c0, max_iter, tol, cdt=np.complex128):
    """Stage 2: ``redundant_refs.solve`` on the derotated block as one unit -- one "frequency" of nfreqs ntimes "times".
    ``c0``: ``(nfeed, nant)``; ``cdt``: the type the derotated block is held in.  Returns ``(c, U, changes, chi2 (nfreqs,
    ntimes), solved (nfeed, nant), vis_solved)``, U and vis_solved in the block's leading shape."""
    nf, nt = d.shape[:2]
    rot = derotate(np.where(gsr.used_weights(d, w, a1, a2) > 0, d, 0), a1, a2, slopes).astype(cdt).astype(np.complex128)
    one = (1, nf * nt) + d.shape[2:]
    ww = np.ones(d.shape) if w is None else np.asarray(w, dtype=np.float64)
    c, U, changes, chi2, solved, vis_solved = rr.solve(rot.reshape(one), ww.reshape(one), np.asarray(c0)[None, None], a1, a2, group,
                                                       ngroups, False, max_iter, tol)
    return (c[0, 0], U.reshape((nf, nt) + U.shape[2:]), changes, chi2.reshape(nf, nt), solved[0, 0],
            vis_solved.reshape((nf, nt) + vis_solved.shape[2:]))


def model_gains(c, tau, freqs):
    """``g[a](nu) = c[a] exp(2 pi i tau[a] (nu - mean(freqs)))`` as the solve's block ``(nfreqs, 1, nfeed, nant)``."""
    nu = np.asarray(freqs, dtype=np.float64)
    return (c[None] * np.exp(2j * np.pi * tau[None] * (nu - nu.mean())[:, None, None]))[:, None]


def firstcal(d, w, a1, a2, group, ngroups, nant, freqs, pad=8, max_iter=200, tol=1e-8, c0=None):
    """Both stages.  Returns a dict: ``gains`` (the solve's block), ``tau``, ``tau_bound``, ``in_pair``, ``c``, ``U``,
    ``changes``, ``chi2``, ``solved``, ``vis_solved``, and stage 1's ``pairs`` dict."""
    nu = np.asarray(freqs, dtype=np.float64)
    nf = len(nu)
    dnu = (nu[-1] - nu[0]) / (nf - 1)
    pair1, pair2 = pairs(group)
    z, _ = products(d, w, a1, a2, pair1, pair2)
    got = pair_delays(z, pad)
    A = pair_matrix(np.asarray(a1), np.asarray(a2), pair1, pair2, nant)
    tau, tau_bound, in_pair = antenna_delays(got["x"], got["used"], got["x_bound"], A, pad * nf, dnu)
    c0 = np.ones(tau.shape, dtype=np.complex128) if c0 is None else c0
    c, U, changes, chi2, solved, vis_solved = offsets(d, w, a1, a2, group, ngroups, 2 * np.pi * tau * dnu, c0, max_iter, tol)
    return dict(gains=model_gains(c, tau, nu), tau=tau, tau_bound=tau_bound, in_pair=in_pair, c=c, U=U, changes=changes, chi2=chi2,
                solved=solved & in_pair, vis_solved=vis_solved, pairs=got, pair1=pair1, pair2=pair2, A=A)
