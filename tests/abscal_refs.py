"""References of abscal (``redundant_abscal``, ``fv_abscal_slopes``, ``fv_abscal_evaluate``) in numpy, straight from the
definitions.  Every stage takes a ``dtype``: ``np.float64`` is the reference, ``np.longdouble`` the variant it is checked against.

Arrays.  ``U``, ``M``, ``W`` are ``(nfreqs, ntimes, ngroups)`` or ``(nfreqs, ntimes, 2, 2, ngroups)`` blocks (``W`` None: ones); ``X``
``(ngroups, ndim)`` holds the groups' baselines in in-plane coordinates, ``ndim`` 1 or 2.  A sample is used when ``W > 0`` and
``X_g != 0``; a flagged sample may be NaN.  A row is a (unit, feed): per-row quantities are ``(nfreqs, ntu, nfeed, ...)`` with
``ntu = ntimes`` for per-time units and 1 otherwise; feed p of a polarized block reads ``[p, p]``.

The model.  ``c_g = sum_t W conj(U) M``, ``S(Phi) = sum_g c_g exp(i Phi . X_g)``, ``N = sum W |U|^2``, ``P = sum W |M|^2``;
``Phi`` maximises ``f = Re S``, ``eta = Re S / N``; gradient ``g = -sum X Im(c e^{i Phi . X})``, Hessian ``H = -sum X X^T Re(c e^{i
Phi . X})``.

Rounding bounds, u = 2^-53, each for ONE implementation (two implementations differ by at most twice as much).

* A strength c_g: nt terms of three products each, added in order: ``|dc_g| <= (nt + 4) u a_g``, ``a_g = sum_t W |U| |M|``.
* One grid value (``e``).  The phase ``theta = phi_1 X_1 + phi_2 X_2`` with ``phi_i = j_i h_i`` is formed with at most two
  roundings per product and one for the sum: ``|dtheta| <= 3 u T``, ``T = |phi_1 X_1| + |phi_2 X_2|``.  The sine and cosine add
  2 u, the product with c 3 u; a run of RUN grid points started by one exact evaluation and continued by RUN - 1 rotations
  by a step factor (its argument, its sine and cosine and the complex product: 6 u a step) adds 6 (RUN - 1) u; this
  reference's ``fast`` variant, which factors ``e^{i theta}`` per dimension, adds one complex product, 3 u, instead.  The sum
  over ngroups terms in any order adds ngroups u.  With the strengths' own error
      ``e = u (ngroups + 3 T_max + 6 RUN + 8 + nt + 4) sum_g a_g``,   ``T_max`` the largest T on the grid.
* ``f``, ``g_i``, ``H_ij`` at a continuous Phi from given strengths (``evaluate``): the terms are ``c e^{i theta}`` times 1, ``X_i``,
  ``X_i X_j``: ``u sum_g |c_g| |X_i|^a |X_j|^b (ngroups + 3 T_g + 12)`` (two more products than e's term, no recurrence).
* The refined slope (``slope_bound``).  A round's step is ``s = -H^-1 g`` where H is negative definite.  With dg and dH the
  bounds above (as 2-norms) and ``lam = min |eig H|``:  ``|ds| <= (|dg| + |dH| |s|) / lam`` per implementation.  A shift B of
  the round's start moves the Newton point by at most ``L B``, ``L = |s| T3 / lam``, ``T3 = sum |c| |X|^3`` bounding the change of
  H per unit of slope (the clip to +-h is 1-Lipschitz).  So ``B <- L B + 2 |ds| + 4 u |Phi|`` over the rounds, from B = 0 at the
  grid point (exact in both); near the maximum s -> 0 and the last round's |ds| remains.  Where H is not safely negative
  definite -- ``H_11 >= -3 dH`` or ``det <= 3 ddet`` -- the rule itself may go either way and the bound is infinite.
"""

import numpy as np

RUN = 8  # the search kernel's run length (ABSCAL_RUN)
U_ROUND = 2.0**-53


def _cdtype(dtype):
    return np.clongdouble if dtype == np.longdouble else np.complex128


def hands(x):
    """The parallel hands of a block as a list of ``(nfreqs, ntimes, ngroups)`` arrays, one per feed."""
    return [x] if x.ndim == 3 else [x[:, :, p, p] for p in range(2)]


def used_weights(U, W, X):
    """``W`` where the sample is used (``W > 0``, ``X_g != 0``), else 0, in the block's shape."""
    w = np.ones(U.shape) if W is None else np.asarray(W, dtype=np.float64)
    return np.where((w > 0) & np.any(np.asarray(X) != 0, axis=1), w, 0.0)


def products(U, M, W, X, per_time, dtype=np.float64):
    """The time-summed strengths per row, times ascending: a dict of ``c``, ``a`` (``sum_t W |U| |M|``), ``Ng``, ``Pg``
    ``(nfreqs, ntu, nfeed, ngroups)``, ``cnt`` (used samples), and the rows' ``N``, ``P`` and ``groups_used``."""
    w = used_weights(U, W, X)
    ok = w > 0
    cd = _cdtype(dtype)
    u, m = np.where(ok, U, 0).astype(cd), np.where(ok, M, 0).astype(cd)
    out = {k: [] for k in ("c", "a", "Ng", "Pg", "cnt")}
    for uf, mf, wf, of in zip(hands(u), hands(m), hands(w.astype(dtype)), hands(ok)):
        terms = dict(c=wf * (np.conj(uf) * mf), a=wf * np.abs(uf) * np.abs(mf), Ng=wf * (uf.real**2 + uf.imag**2),
                     Pg=wf * (mf.real**2 + mf.imag**2), cnt=of.astype(np.int64))
        for k, t in terms.items():
            if per_time:
                out[k].append(t)
            else:
                s = np.zeros_like(t[:, :1])
                for i in range(t.shape[1]):
                    s[:, 0] += t[:, i]
                out[k].append(s)
    out = {k: np.stack(v, axis=2) for k, v in out.items()}
    out["N"], out["P"] = out["Ng"].sum(axis=-1), out["Pg"].sum(axis=-1)
    out["groups_used"] = (out["cnt"] > 0).sum(axis=-1)
    return out


def grid_axes(n, h, dtype=np.float64):
    """``phi_i = (i - (n_i - 1) / 2) h_i``: two arrays."""
    return [(np.arange(n[i]) - (n[i] - 1) // 2).astype(dtype) * dtype(h[i]) for i in range(2)]


def _xy(X, dtype):
    X = np.asarray(X, dtype=dtype)
    return X[:, 0], X[:, 1] if X.shape[1] == 2 else np.zeros(len(X), dtype=dtype)


def grid_values(c, X, n, h, dtype=np.float64, fast=False):
    """``Re S`` on the grid for every row of ``c`` ``(..., ngroups)``: ``(..., n_1, n_2)``."""
    c = np.asarray(c).astype(_cdtype(dtype))
    p1, p2 = grid_axes(n, h, dtype)
    x1, x2 = _xy(X, dtype)
    rows = c.reshape(-1, c.shape[-1])
    out = np.zeros((len(rows), n[0], n[1]), dtype=dtype)
    if fast:
        e2 = np.exp(1j * np.outer(x2, p2))  # (ngroups, n2)
        for i in range(n[0]):
            out[:, i] = ((rows * np.exp(1j * p1[i] * x1)) @ e2).real
    else:
        for i in range(n[0]):
            theta = (p1[i] * x1)[:, None] + np.outer(x2, p2)
            out[:, i] = rows.real @ np.cos(theta) - rows.imag @ np.sin(theta)
    return out.reshape(c.shape[:-1] + (n[0], n[1]))


def value_bound(a, X, n, h, nt=1):
    """``e`` of the module's docstring for every row of ``a`` ``(..., ngroups)`` (``sum_t W |U| |M|``, or ``|c|`` with ``nt = 0`` for
    strengths that are given, not formed)."""
    X = np.abs(np.asarray(X, dtype=np.float64))
    t_max = sum(X[:, i].max(initial=0.0) * ((n[i] - 1) // 2) * h[i] for i in range(X.shape[1]))
    return U_ROUND * (a.shape[-1] + 3 * t_max + 6 * RUN + 8 + nt + 4) * np.asarray(a, dtype=np.float64).sum(axis=-1)


def search(c, X, n, h, dtype=np.float64, fast=False):
    """The grid and its argmax, the lowest flat index ``i_1 n_2 + i_2`` among equal maxima: ``(values, flat, j)`` with ``j``
    ``(..., 2)`` the signed steps of the peak."""
    y = grid_values(c, X, n, h, dtype, fast)
    flat = np.argmax(y.reshape(y.shape[:-2] + (-1,)), axis=-1)
    j = np.stack([flat // n[1] - (n[0] - 1) // 2, flat % n[1] - (n[1] - 1) // 2], axis=-1)
    return y, flat, j


def evaluate(c, X, phi, dtype=np.float64, a=None, extra=0.0):
    """``f, g_1, g_2, H_11, H_12, H_22`` at the continuous ``phi`` ``(..., 2)`` for the rows of ``c`` ``(..., ngroups)``, and
    their bounds: two arrays ``(..., 6)``.  For strengths that were formed from blocks, not given, ``a`` (``sum_t W |U| |M|``,
    in place of ``|c|``) and ``extra = nt + 4`` add their own error to the bounds."""
    cc = np.asarray(c).astype(_cdtype(dtype))
    x1, x2 = _xy(X, dtype)
    phi = np.asarray(phi, dtype=dtype)
    theta = phi[..., :1] * x1 + phi[..., 1:2] * x2
    w = cc * np.exp(1j * theta)
    mono = [np.ones_like(x1), x1, x2, x1 * x1, x1 * x2, x2 * x2]
    part = [w.real, -w.imag, -w.imag, -w.real, -w.real, -w.real]
    s = np.stack([(p * m).sum(axis=-1) for p, m in zip(part, mono)], axis=-1)
    t = (np.abs(phi[..., :1] * x1) + np.abs(phi[..., 1:2] * x2)).astype(np.float64)
    k = cc.shape[-1] + 3 * t + 12 + extra
    mag = np.abs(cc).astype(np.float64) if a is None else np.asarray(a, dtype=np.float64)
    bound = np.stack([U_ROUND * (mag * np.abs(m).astype(np.float64) * k).sum(axis=-1) for m in mono], axis=-1)
    return s, bound


def newton_step(s, ndim, h):
    """The rule's step for one row from its six sums, clipped to +-h: ``(step (2,), definite)``."""
    f, g1, g2, h11, h12, h22 = s
    zero = s[0] * 0
    if ndim == 1:
        d = [-g1 / h11 if h11 < 0 else (g1 / h11 if h11 > 0 else zero), zero]
        definite = h11 < 0
    else:
        det = h11 * h22 - h12 * h12
        definite = h11 < 0 and det > 0
        if definite:
            d = [-(h22 * g1 - h12 * g2) / det, -(h11 * g2 - h12 * g1) / det]
        else:
            hd = (h11 - h22) / 2
            big = abs((h11 + h22) / 2) + np.sqrt(hd * hd + h12 * h12)
            d = [g1 / big if big > 0 else zero, g2 / big if big > 0 else zero]
    return np.array([np.clip(d[0], -h[0], h[0]), np.clip(d[1], -h[1], h[1]) if ndim == 2 else zero]), definite


def refine(c, X, j, h, rounds, dtype=np.float64, a=None, extra=0.0):
    """``rounds`` of the Newton rule from the grid points ``j`` ``(..., 2)`` (signed steps): ``(phi (..., 2), slope_bound (...),
    s (..., 6))``, ``s`` the sums of one more evaluation at the result."""
    ndim = np.asarray(X).shape[1]
    cc = np.asarray(c)
    lead = cc.shape[:-1]
    rows = cc.reshape(-1, cc.shape[-1])
    mags = np.abs(rows).astype(np.float64) if a is None else np.asarray(a, dtype=np.float64).reshape(rows.shape)
    jj = np.asarray(j).reshape(-1, 2)
    hh = [dtype(h[0]), dtype(h[1])]
    phi = np.zeros((len(rows), 2), dtype=dtype)
    bound = np.zeros(len(rows))
    last = np.zeros((len(rows), 6), dtype=dtype)
    r3 = (np.abs(np.asarray(X, dtype=np.float64)) ** 2).sum(axis=1) ** 1.5
    for r, cr in enumerate(rows):
        p = np.array([dtype(jj[r, 0]) * hh[0], dtype(jj[r, 1]) * hh[1] if ndim == 2 else dtype(0)], dtype=dtype)
        t3 = float((mags[r] * r3).sum())
        b = 0.0
        for _ in range(rounds):
            s, sb = evaluate(cr, X, p, dtype, mags[r], extra)
            step, definite = newton_step(s, ndim, hh)
            sf, sbf = s.astype(np.float64), sb.astype(np.float64)
            if ndim == 1:
                lam, safe = abs(sf[3]), sf[3] < -3 * sbf[3]
                dg, dh = sbf[1], sbf[3]
            else:
                det = sf[3] * sf[5] - sf[4] ** 2
                ddet = abs(sf[3]) * sbf[5] + abs(sf[5]) * sbf[3] + 2 * abs(sf[4]) * sbf[4]
                lam = abs(abs((sf[3] + sf[5]) / 2) - np.hypot((sf[3] - sf[5]) / 2, sf[4]))
                safe = sf[3] < -3 * sbf[3] and det > 3 * ddet
                dg, dh = np.hypot(sbf[1], sbf[2]), np.sqrt(sbf[3] ** 2 + 2 * sbf[4] ** 2 + sbf[5] ** 2)
            if not (np.isfinite(b) and definite and safe and lam > 0):
                b = np.inf
            else:
                ns = float(np.hypot(*step.astype(np.float64)))
                b = ns * t3 / lam * b + 2 * (dg + dh * ns) / lam + 4 * U_ROUND * float(np.abs(p).sum())
            p = p + step
        phi[r], bound[r] = p, b
        last[r] = evaluate(cr, X, p, dtype)[0]
    return phi.reshape(lead + (2,)), bound.reshape(lead), last.reshape(lead + (6,))


def chi2_rows(U, M, W, X, amp, phi, per_time):
    """``sum W |eta e^{-i Phi . X} U - M|^2`` per (frequency, time) over the feeds and the used samples, ``amp`` ``(nfreqs, ntu,
    nfeed)`` and ``phi`` ``(nfreqs, ntu, nfeed, 2)`` per row; also ``sum W |eta U|^2`` and the largest ``|phi_1 X_1| + |phi_2 X_2|``:
    ``(chi2, power, t_max)``."""
    w = used_weights(U, W, X)
    ok = w > 0
    x1, x2 = _xy(X, np.float64)
    chi2 = np.zeros(U.shape[:2])
    power = np.zeros(U.shape[:2])
    t_max = 0.0
    for p, (uf, mf, wf, of) in enumerate(zip(hands(np.where(ok, U, 0)), hands(np.where(ok, M, 0)), hands(w), hands(ok))):
        a, ph = amp[:, :, p], phi[:, :, p]  # (nfreqs, ntu[, 2]): broadcast over the times of a time-constant unit
        theta = ph[..., :1] * x1 + ph[..., 1:2] * x2
        v = a[..., None] * np.exp(-1j * theta) * uf
        chi2 += (wf * np.abs(v - mf) ** 2).sum(axis=-1)
        power += (wf * np.abs(v) ** 2).sum(axis=-1)
        t_max = max(t_max, float((np.abs(ph[..., :1] * x1) + np.abs(ph[..., 1:2] * x2)).max(initial=0.0)))
    return chi2, power, t_max


def chi2_bound(chi2, power, t_max, L):
    """The absolute bound of a reported chi2 against ``chi2_rows`` at the same parameters, per (f, t).  Both form ``v = eta
    e^{-i theta} U`` in fp64 from the same inputs: the phase, the sine and cosine and three products put it within ``k u |v|``,
    ``k = 3 t_max + 9``, on either side, the subtraction adds ``u |delta|``; a term ``W |delta|^2`` is then off by at most ``2 W
    |delta| k u |v| + W (k u |v|)^2`` on either side, by Cauchy-Schwarz the row by ``4 k u sqrt(power chi2) + 2 (k u)^2 power``,
    and the two summation orders and the terms' own roundings add ``(L + 6) 2^-52 chi2``."""
    k = 3 * t_max + 9
    return (L + 6) * 2.0**-52 * chi2 + 4 * k * U_ROUND * np.sqrt(power * chi2) + 2 * (k * U_ROUND) ** 2 * power


def abscal(U, M, W, X, n, h, rounds, per_time, dtype=np.float64, peak=None, fast=False):
    """The whole fit.  ``peak``: grid points ``(..., 2)`` to refine from in place of the search's (another implementation's,
    where two grid values are equal within ``e``).  Returns a dict: ``prod`` (``products``), ``y``, ``flat``, ``j``, ``e``, ``phi``,
    ``slope_bound``, ``amp``, ``power``, ``N``, ``P``, ``used``, ``peak`` (0 where not used), ``chi2``, ``sums`` (the last evaluation)."""
    ndim = np.asarray(X).shape[1]
    prod = products(U, M, W, X, per_time, dtype)
    y, flat, j = search(prod["c"], X, n, h, dtype, fast)
    e = value_bound(prod["a"], X, n, h, nt=1 if per_time else U.shape[1])
    start = j if peak is None else np.asarray(peak)
    phi, bound, s = refine(prod["c"], X, start, h, rounds, dtype, prod["a"], (1 if per_time else U.shape[1]) + 4)
    f = s[..., 0]
    used = (prod["N"] > 0) & (prod["groups_used"] >= ndim + 1) & (f > 0)
    amp = np.where(used, f / np.where(used, prod["N"], 1), 1)
    phi = np.where(used[..., None], phi, 0)
    chi2 = chi2_rows(U, M, W, X, amp.astype(np.float64), phi.astype(np.float64), per_time)[0]
    return dict(prod=prod, y=y, flat=flat, j=j, e=e, phi=phi, slope_bound=np.where(used, bound, 0.0), amp=amp, power=np.where(used, f, 0),
                N=prod["N"], P=prod["P"], used=used, peak=np.where(used[..., None], start, 0), chi2=chi2, sums=s)


def plane(b):
    """The plane of the baselines ``b`` ``(ngroups, 3)``: ``(Vt (ndim, 3), X (ngroups, ndim))``, the right singular vectors whose
    singular value exceeds 1e-9 of the largest."""
    cross = np.any(b != 0, axis=1)
    _, s, vt = np.linalg.svd(b[cross], full_matrices=False)
    vt = vt[: max(1, int((s > 1e-9 * s[0]).sum()))]
    X = b @ vt.T
    X[~cross] = 0
    return vt, X


def grid(X, b, pad, max_slope=None):
    """``(n, h, max_slope)`` of the search: ``h_i = 2 pi / (pad extent_i)``, ``n_i = 2 ceil(max_slope / h_i) + 1``, ``max_slope``
    by default ``pi / min |b|``; ``n_2 = 1`` for a line."""
    cross = np.any(b != 0, axis=1)
    if max_slope is None:
        max_slope = np.pi / np.sqrt((b[cross] ** 2).sum(axis=1)).min()
    n, h = [1, 1], [1.0, 1.0]
    for i in range(X.shape[1]):
        extent = X[cross, i].max() - X[cross, i].min()
        extent = extent if extent > 0 else np.abs(X[cross, i]).max()
        h[i] = 2 * np.pi / (pad * extent)
        n[i] = 2 * int(np.ceil(max_slope / h[i])) + 1
    return n, h, float(max_slope)


def apply(gains, amp, slopes, pos, used):
    """The gains' block ``(nfreqs, ntu, nfeed, nant)`` times ``eta^-1/2 exp(i Phi . (x_a - mean x))`` where the row is used;
    ``slopes`` ``(nfreqs, ntu, nfeed, 3)`` in the antennas' frame, ``pos`` ``(nant, 3)``."""
    factor = np.exp(1j * (slopes @ (pos - pos.mean(axis=0)).T)) / np.sqrt(amp)[..., None]
    return np.where(used[..., None], gains * factor, gains)
