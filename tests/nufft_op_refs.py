"""References and bounds for the element-wise tests of the type-3 transform op (``gpu_nufft2d`` / ``gpu_nufft3d`` /
``gpu_nudft_direct``).  CPU only; nothing here touches the device.

Three things are compared, element by element and row by row:

* ``exact_type3``: the direct sum in extended precision, the truth;
* ``port``: ``oracle.cpu_nufft.nufft_type3``, a CPU realisation of the same published algorithm with the same kernel
  rule as ``fv_eskernel.h`` -- its own error against the truth sets the tolerance (``bound``);
* the device's result, held to ``bound`` in ``tests/test_gpu_nufft_elementwise.py``.

The metric is ``element_ratio``: ``|got - exact| / (eps ||c_t||_2)`` per transform ``t`` and target ``k`` -- the scale is
the transform's own, so a row of small strengths beside large ones is measured against itself, and one target is not
averaged away by the other 299.  ``row_rel_l2`` is the rel l2 of every row against its own exact row."""

import functools
import json
import os

import numpy as np

from oracle import cpu_nufft, nudft

EXTENDED = np.finfo(np.longdouble).nmant >= 63  # an 80-bit (or wider) long double

EPS_SIGMA2 = (1e-3, 1e-6, 1e-9, 1e-12)
EPS_SIGMA125 = (1e-3, 1e-6, 1e-8)  # fv_eskernel.h: ~1e-8 is this sigma's fp64 floor


def unit_roundoff(precision):
    return 2.0**-53 if precision == 2 else 2.0**-24


# ---------------------------------------------------------------------------------------------------------------------
# The exact sum
# ---------------------------------------------------------------------------------------------------------------------
def exact_type3(coords, c, targets):
    """``f[t, k] = sum_j c[t, j] exp(+i s_k . x_j)`` as ``(re, im)`` in ``numpy.longdouble``: the phases by outer products,
    their cos / sin, two real matrix products.  With a 64-bit mantissa the phases carry 2^-64 Phi instead of 2^-53 Phi, which
    is what makes a comparison at eps = 1e-12 mean something (the fp64 oracle sits at up to 0.66 of that eps).  Where long
    double is no wider than double the fp64 oracle's sum is returned (``floor`` then counts its phase term twice)."""
    c = np.atleast_2d(np.asarray(c))
    if not EXTENDED:
        f = nudft.nudft_type3([np.asarray(a, float) for a in coords], c.astype(complex),
                              [np.asarray(a, float) for a in targets])
        return f.real.astype(np.longdouble), f.imag.astype(np.longdouble)
    ld = np.longdouble
    ph = sum(np.multiply.outer(np.asarray(s, dtype=ld), np.asarray(x, dtype=ld)) for x, s in zip(coords, targets))
    cs = np.concatenate([np.cos(ph), np.sin(ph)], axis=1)  # (N, 2M)
    cr, ci = c.real.astype(ld), c.imag.astype(ld)
    re = np.concatenate([cr, -ci], axis=1) @ cs.T
    im = np.concatenate([ci, cr], axis=1) @ cs.T
    return re, im


def port(coords, c, targets, eps, sigma):
    """The CPU port of the published algorithm (C kernels in 2-D, numpy in 3-D), in fp64."""
    return cpu_nufft.nufft_type3([np.asarray(a, float) for a in coords], np.atleast_2d(c).astype(complex),
                                 [np.asarray(a, float) for a in targets], eps=eps, sigma=sigma)


# ---------------------------------------------------------------------------------------------------------------------
# Metrics
# ---------------------------------------------------------------------------------------------------------------------
def _err(got, exact):
    re, im = exact
    got = np.atleast_2d(np.asarray(got))
    return np.hypot(got.real.astype(np.longdouble) - re, got.imag.astype(np.longdouble) - im).astype(float)


def row_norms(c):
    c = np.atleast_2d(np.asarray(c)).astype(complex)
    return np.abs(c).sum(axis=1), np.sqrt((np.abs(c) ** 2).sum(axis=1))


def element_ratio(got, exact, c, eps):
    """``|got - exact| / (eps ||c_t||_2)``, shape (ntrans, N): every row against its own strengths."""
    return _err(got, exact) / (eps * row_norms(c)[1][:, None])


def row_rel_l2(got, exact):
    """rel l2 of every row against its own exact row, shape (ntrans,)."""
    re, im = exact
    den = np.sqrt((re.astype(float) ** 2 + im.astype(float) ** 2).sum(axis=1))
    return np.sqrt((_err(got, exact) ** 2).sum(axis=1)) / np.where(den > 0, den, 1.0)


def whole_rel_l2(got, exact):
    """The metric of the older op tests: one rel l2 over the whole (ntrans, N) array."""
    re, im = exact
    return float(np.sqrt((_err(got, exact) ** 2).sum() / (re.astype(float) ** 2 + im.astype(float) ** 2).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# The rounding a correct kernel cannot avoid
# ---------------------------------------------------------------------------------------------------------------------
def max_phase(case):
    """Phi = sum_d max_j |x_dj| max_k |s_dk|: the largest phase the inputs can form."""
    return float(sum(np.abs(x).max() * np.abs(s).max() for x, s in zip(case["coords"], case["targets"])))


def phase_term(case, precision=None):
    """Term 1 of ``floor`` as an absolute error per row, shape (ntrans,)."""
    u = unit_roundoff(case["precision"] if precision is None else precision)
    d = len(case["coords"])
    return (2 * d - 1) * u * max_phase(case) * row_norms(case["c"])[0]


def fft_term(case, eps, sigma, precision=None):
    """Term 2 of ``floor`` as an absolute error per (t, k), shape (ntrans, N): ``u (sum_d log2 n2_d) A_k ||c_t||_2``, the
    rounding of the FFT stage alone as it reaches target k (derived under ``floor``).  tests/fft_stage_refs.py holds the
    difference of two realisations of the FFT to a multiple of this."""
    u = unit_roundoff(case["precision"] if precision is None else precision)
    l2 = row_norms(case["c"])[1]
    w, beta = cpu_nufft.es_params(eps, sigma)
    hat0 = float(cpu_nufft.es_hat(np.zeros(1), w, beta)[0])
    amp, stages = np.ones(case["targets"][0].size), 0.0
    for x, s in zip(case["coords"], case["targets"]):
        x, s = np.asarray(x, float), np.asarray(s, float)
        xc, sc = 0.5 * (x.min() + x.max()), 0.5 * (s.min() + s.max())
        _, n2, h = cpu_nufft._geom(np.abs(x - xc).max(), np.abs(s - sc).max(), sigma, w)
        amp *= hat0 / cpu_nufft.es_hat(h * (s - sc), w, beta)
        stages += np.log2(n2)
    return u * stages * amp[None, :] * l2[:, None]


def floor(case, eps, sigma, precision=None):
    """Per (t, k), in units of ``eps ||c_t||_2``: the rounding error that a correct transform working in ``precision``
    (unit roundoff u = 2^-53 or 2^-24) cannot avoid.  Two terms, both derived:

    1. Phase formation.  The phase of source j at target k is ``sum_d s_dk x_dj``: d products and d - 1 additions, each
       rounded once, so the computed phase is off by at most ``(2d - 1) u max|phase| <= (2d - 1) u Phi`` with
       ``Phi = sum_d max_j |x_dj| max_k |s_dk|`` (centring the boxes first only moves where the same products are formed:
       the pre- and post-phases carry them).  ``|d/dphase exp(i phase)| = 1``, so the term of source j moves by at most
       that times ``|c_tj|``; summed over the sources by the triangle inequality: ``(2d - 1) u Phi ||c_t||_1``.

    2. The FFT (``fft_term``).  A transform of length n done in log2 n radix-2 stages leaves a relative l2 error of
       ``u log2 n`` per dimension (each stage rounds every entry once), i.e. ``u sum_d log2 n2_d`` of the grid's norm per
       entry on the average; the spread grid's Fourier content is ``||c_t||_2`` per mode up to the kernel's normalisation,
       which the final division by the kernel's transform undoes at the centre of the band and OVER-undoes away from it: a
       target at ``s'`` (centred) is divided by ``psi_hat(h_d s'_d)`` per dimension where the signal it carries was only
       multiplied by that much, but the FFT's rounding noise was not.  So the noise reaches the output multiplied by
       ``A_k = prod_d psi_hat(0) / psi_hat(h_d s'_dk)``: ``u (sum_d log2 n2_d) A_k ||c_t||_2``.  ``A_k`` is 1 at the
       centre of the target box and largest in its corners (sigma = 2: ~e^{0.14 w} per dimension; sigma = 1.25:
       ~e^{w/2}), which is the "amplified rounding at band-edge targets" of ``fv_eskernel.h``.

    Width, shape and grid come from the port's ``es_params`` / ``_geom``; where long double is no wider than double,
    term 1 is counted twice (the reference's own phases)."""
    precision = case["precision"] if precision is None else precision
    l2 = row_norms(case["c"])[1]
    t1 = phase_term(case, precision) * (1 if EXTENDED else 2)
    return (t1[:, None] + fft_term(case, eps, sigma, precision)) / (eps * l2[:, None])


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
def _box_points(half, centre=None):
    """The corners, then (2-D) the edge midpoints and the centre of a box: exact extremes, no draw decides them."""
    d = len(half)
    centre = [0.0] * d if centre is None else centre
    pts = [[sx * half[0], sy * half[1]] + ([sz * half[2]] if d == 3 else [])
           for sx in (-1, 1) for sy in (-1, 1) for sz in ((-1, 1) if d == 3 else (0,))]
    ncorner = len(pts)
    if d == 2:
        pts += [[-half[0], 0.0], [half[0], 0.0], [0.0, -half[1]], [0.0, half[1]], [0.0, 0.0]]
    return np.array(pts).T + np.array(centre)[:, None], ncorner


def _make(dim, M, N, X, S, ntrans, seed, corners=False, scales=False, cluster=False, shift=None, precision=2,
          xlo=None, eps=None, disc=False):
    """A seeded problem: sources uniform in the box of half-widths ``X`` (``xlo``: lower ends instead of -X), targets
    uniform in that of half-widths ``S``; ``corners``: the extreme points of both boxes put in front; ``cluster``: 150
    sources drawn into one bin; ``scales``: rows of c times 10^linspace(-6, 6, ntrans); ``shift``: both boxes moved;
    ``disc``: the targets in the ellipse inscribed in their box instead; ``eps``: the tolerances per sigma where they are not the precision's whole list."""
    rng = np.random.default_rng(seed)
    X, S = np.broadcast_to(np.asarray(X, float), (dim,)), np.broadcast_to(np.asarray(S, float), (dim,))
    lo = -X if xlo is None else np.asarray(xlo, float)
    x = lo[:, None] + (X - lo)[:, None] * rng.uniform(0, 1, (dim, M))
    s = S[:, None] * rng.uniform(-1, 1, (dim, N))
    if disc:  # targets in the ellipse inscribed in the box, its four axis points included: none in a corner
        r, a = np.sqrt(rng.uniform(0, 1, N)), rng.uniform(0, 2 * np.pi, N)
        s = S[:, None] * np.array([r * np.cos(a), r * np.sin(a)])
        s[:, :4] = S[:, None] * np.array([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, -1.0]])
    c = rng.normal(size=(ntrans, M)) + 1j * rng.normal(size=(ntrans, M))
    kind = np.zeros(N, dtype=int)  # 0 interior, 1 corner, 2 edge midpoint / centre
    if cluster:
        n = min(150, M)
        x[:, :n] = x[:, :1] + 1e-3 * (x[:, :n] - x[:, :1])
    if corners:
        half, mid = 0.5 * (X - lo), 0.5 * (X + lo)
        px, nc = _box_points(half, mid)
        x[:, -nc:] = px[:, :nc]  # (at the end: the cluster keeps the front)
        ps, nc = _box_points(S)
        s[:, :ps.shape[1]] = ps
        kind[:nc], kind[nc:ps.shape[1]] = 1, 2
    if scales:
        c = c * 10.0 ** np.linspace(-6, 6, ntrans)[:, None]
    if shift is not None:
        x = x + np.asarray(shift[0], float)[:, None]
        s = s + np.asarray(shift[1], float)[:, None]
    if precision == 1:  # the inputs ARE float32 numbers: every reference works on exactly these
        x, s, c = x.astype(np.float32), s.astype(np.float32), c.astype(np.complex64)
    for a in (x, s, c, kind):
        a.setflags(write=False)
    fam = {2: "2d_plain", 3: "3d_plain"}[dim] + ("32" if precision == 1 else "")
    return {"dim": dim, "coords": list(x), "targets": list(s), "c": c, "kind": kind, "precision": precision,
            "plain": fam, "eps": eps}


_PLAIN2 = dict(dim=2, M=400, N=300, X=3.0, S=60.0, ntrans=5)
_P3 = dict(dim=3, M=200, N=150, ntrans=3)
# Which tolerances a case runs at is decided by ``floor``, never by a result: a combination whose floor passes 5 units
# somewhere would bring a lax bound with it (tests/test_nufft_op_host.py asserts the cap for every combination).
# Phi of several hundred and more: term 1 alone passes 5 units at eps = 1e-12.
_GE9 = {2.0: EPS_SIGMA2[:3], 1.25: EPS_SIGMA125}
# Exact corners in 3-D at sigma = 1.25 and eps = 1e-8 (w = 15): A_k = e^{~22} there and term 2 is ~300 units.  The plain
# 3-D case keeps 1e-8 (3.2 units at its outermost target).
_CORNERS3 = {2.0: EPS_SIGMA2, 1.25: EPS_SIGMA125[:2]}
# fp32 (the floors the Nufft3 constructor states: sigma 2 at 1e-3 and 1e-4; sigma 1.25 at 1e-4 in 2-D, 1e-3 in 3-D).
# An exact 2-D corner at sigma = 1.25 and 1e-4 (w = 8) has A_k = e^{~8}: term 2 is ~8 units in fp32, so the fp32 corner
# case runs at sigma 2 only and the fp32 plain case draws its targets in the ellipse inscribed in the box (its four
# axis points included): band edge in one dimension at a time, 1.6 units.
_FP32_2D = {2.0: (1e-3, 1e-4), 1.25: (1e-4,)}
_FP32_2D_CORNERS = {2.0: (1e-3, 1e-4), 1.25: ()}
_FP32_3D = {2.0: (1e-3, 1e-4), 1.25: (1e-3,)}
_RECIPES = {
    "2d_plain": dict(_PLAIN2, seed=101),
    "2d_corners": dict(_PLAIN2, seed=102, corners=True),
    "2d_rowscales_5": dict(_PLAIN2, seed=103, corners=True, scales=True, cluster=True),
    "2d_rowscales_19": dict(_PLAIN2, seed=104, corners=True, scales=True, cluster=True, ntrans=19),
    "2d_rowscales_24": dict(_PLAIN2, seed=105, corners=True, scales=True, cluster=True, ntrans=24),
    "2d_tiny_16x5": dict(dim=2, M=400, N=300, X=1.21, S=(16.75, 5.1), ntrans=2, seed=120, corners=True),
    "2d_tiny_8x8": dict(dim=2, M=400, N=300, X=0.6, S=8.0, ntrans=2, seed=121, corners=True),
    "2d_offcentre": dict(_PLAIN2, seed=130, shift=((11.0, -7.0), (300.0, -120.0)), eps=_GE9),
    "2d_zero_extent": dict(_PLAIN2, seed=140, X=(3.0, 0.0), S=(60.0, 0.0), xlo=(-3.0, 0.0)),
    "2d_narrow_source_box": dict(_PLAIN2, seed=141, X=0.5e-6),
    "2d_one_source": dict(_PLAIN2, seed=142, M=1),
    "2d_one_target": dict(_PLAIN2, seed=143, N=1),
    "2d_coincident": dict(dim=2, M=50, N=30, X=(1.25, -0.5), xlo=(1.25, -0.5), S=0.0, ntrans=2, seed=144,
                          shift=((0.0, 0.0), (3.0, 4.0))),
    "3d_plain": dict(_P3, seed=201, X=2.0, S=10.0),
    "3d_cubic": dict(_P3, seed=202, X=2.0, S=10.0, corners=True, eps=_CORNERS3),
    "3d_thin": dict(_P3, seed=203, X=2.0, S=(10.0, 10.0, 1.5), xlo=(-2.0, -2.0, 0.0), corners=True,
                    eps=_CORNERS3),
    # fp32: Phi <= 60 and M <= 200, so that term 1 stays below 2 units at eps = 1e-4
    "2d_plain32": dict(dim=2, M=200, N=300, X=3.0, S=10.0, ntrans=5, seed=301, precision=1, disc=True, eps=_FP32_2D),
    "2d_corners32": dict(dim=2, M=200, N=300, X=3.0, S=10.0, ntrans=5, seed=302, precision=1, corners=True,
                         eps=_FP32_2D_CORNERS),
    "3d_plain32": dict(dim=3, M=150, N=150, X=2.0, S=8.0, ntrans=3, seed=303, precision=1, eps=_FP32_3D),
    "3d_corners32": dict(dim=3, M=150, N=150, X=2.0, S=8.0, ntrans=3, seed=304, precision=1, corners=True,
                         eps=_FP32_3D),
}
for _i, (_sx, _sy) in enumerate([(700, 20), (62, 256), (256, 62), (390, 200), (520, 128)]):
    _RECIPES[f"2d_aniso_{_sx}x{_sy}"] = dict(dim=2, M=400, N=300, X=3.0, S=(float(_sx), float(_sy)), ntrans=2,
                                             seed=110 + _i, corners=True, eps=_GE9)
CASES = tuple(_RECIPES)
CASES_FP64_2D = tuple(n for n in CASES if n.startswith("2d") and not n.endswith("32"))
CASES_FP64_3D = ("3d_plain", "3d_cubic", "3d_thin")
CASES_FP32 = tuple(n for n in CASES if n.endswith("32"))
# (family's plain case, sigma, the eps a run at 100 eps is judged at): every (dimension, precision, sigma) of the op tests
SENSITIVITY = (("2d_plain", 2.0, 1e-6), ("2d_plain", 1.25, 1e-6), ("3d_plain", 2.0, 1e-6), ("3d_plain", 1.25, 1e-6),
               ("2d_plain32", 2.0, 1e-4), ("2d_plain32", 1.25, 1e-4), ("3d_plain32", 2.0, 1e-4),
               ("3d_plain32", 1.25, 1e-3))


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded problem ``name`` (read-only arrays, built once): ``coords``, ``targets`` (lists of d arrays), ``c``
    (ntrans, M), ``kind`` per target (0 interior, 1 corner, 2 edge midpoint or centre), ``precision``, ``plain`` (the
    yardstick case of its family).  A recipe's ``make`` names another builder than ``_make`` (tests/fft_stage_refs.py
    registers its dense cases here, so that ``exact`` / ``bound`` / ``check`` serve them unchanged)."""
    recipe = dict(_RECIPES[name])
    return dict(recipe.pop("make", _make)(**recipe), name=name)


def eps_list(name, sigma):
    """The tolerances a case runs at: its recipe's, or the whole fp64 list of the sigma."""
    cs = case(name)
    if cs["eps"] is not None:
        return cs["eps"][sigma]
    return EPS_SIGMA2 if sigma == 2.0 else EPS_SIGMA125


def combos(names):
    return [(n, eps, sigma) for n in names for sigma in (2.0, 1.25) for eps in eps_list(n, sigma)]


@functools.lru_cache(maxsize=None)
def exact(name):
    cs = case(name)
    re, im = exact_type3(cs["coords"], cs["c"], cs["targets"])
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


@functools.lru_cache(maxsize=None)
def port_result(name, eps, sigma):
    cs = case(name)
    out = port(cs["coords"], cs["c"], cs["targets"], eps, sigma)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The bound
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def port_worst(name, eps, sigma):
    """The port's worst element ratio on a case (Y) and its rel l2 per row."""
    cs = case(name)
    out = port_result(name, eps, sigma)
    return float(element_ratio(out, exact(name), cs["c"], eps).max()), row_rel_l2(out, exact(name))


@functools.lru_cache(maxsize=None)
def bound(name, eps, sigma):
    """What a result on case ``name`` at ``(eps, sigma)`` is held to -- measured on the reference, never on the device:

        element_ratio[t, k] <= 2 max(Y_case, Y_plain) + floor[t, k]
        row_rel_l2[t]       <= max(5 eps, 2 port's row_rel_l2[t]) + ||floor[t, :]|| (as a rel l2 of that row)

    ``Y_case`` / ``Y_plain``: the port's worst element ratio on this case / on the plain case of its family (dimension
    and precision; the sigma is the run's).  The margin of 2 is the project's rule for every bound (tests/helpers.py) and
    covers two correct realisations of the same approximation on different fine grids; 5 eps is the op's stated
    contract.  fp32 cases: the port runs in fp64 on the rounded inputs."""
    cs = case(name)
    y_case, port_rows = port_worst(name, eps, sigma)
    y_plain = port_worst(cs["plain"], eps, sigma)[0]
    fl = floor(cs, eps, sigma)
    re, im = exact(name)
    den = np.sqrt((re.astype(float) ** 2 + im.astype(float) ** 2).sum(axis=1))
    fl_rows = np.sqrt(((fl * eps * row_norms(cs["c"])[1][:, None]) ** 2).sum(axis=1)) / np.where(den > 0, den, 1.0)
    return {"Y_case": y_case, "Y_plain": y_plain, "floor": fl, "element": 2.0 * max(y_case, y_plain) + fl,
            "port_rows": port_rows, "rows": np.maximum(5 * eps, 2.0 * port_rows) + fl_rows}


def judge(got, name, eps, sigma, rows=None, label="", path=""):
    """A result on case ``name`` against ``bound(name, eps, sigma)``: the metrics, where the worst element fell and
    the two verdicts (``ok_element``, ``ok_rows``) -- no assertion.  ``rows``: ``got[i]`` is the transform of row
    ``rows[i]`` of the case's strengths (a permutation test).  Logged as one JSON line when FFTVIS_TEST_METRICS is set."""
    cs, b = case(name), bound(name, eps, sigma)
    rows = np.arange(cs["c"].shape[0]) if rows is None else np.asarray(rows)
    re, im = exact(name)
    ex = (re[rows], im[rows])
    ratio = element_ratio(got, ex, cs["c"][rows], eps)
    rl2 = row_rel_l2(got, ex)
    finite = bool(np.isfinite(np.asarray(got).view(np.asarray(got).real.dtype)).all())
    over = np.where(np.isfinite(ratio), ratio, np.inf) - b["element"][rows]
    t, k = np.unravel_index(int(np.argmax(over)), over.shape)
    tw, kw = np.unravel_index(int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf))), ratio.shape)
    m = {"case": name, "eps": eps, "sigma": sigma, "precision": cs["precision"], "path": path, "label": label,
         "worst_ratio": float(ratio[tw, kw]), "worst_at": [int(rows[tw]), int(kw)],
         "worst_kind": ("interior", "corner", "edge")[int(cs["kind"][kw])],
         "worst_margin": float(over[t, k]), "worst_margin_at": [int(rows[t]), int(k)],
         "worst_row_rel_l2_in_eps": float((rl2 / eps).max()), "worst_row": int(rows[int(np.argmax(rl2))]),
         "port_worst_row_rel_l2_in_eps": float((b["port_rows"] / eps).max()),
         "Y_case": b["Y_case"], "Y_plain": b["Y_plain"], "floor_max": float(b["floor"].max()),
         "ok_element": bool(finite and (over <= 0).all()),
         "ok_rows": bool(finite and (rl2 <= b["rows"][rows]).all())}
    if os.environ.get("FFTVIS_TEST_METRICS"):
        with open(os.environ["FFTVIS_TEST_METRICS"], "a") as f:
            f.write(json.dumps(dict(m, test=os.environ.get("PYTEST_CURRENT_TEST", ""))) + "\n")
    return m


def check(got, name, eps, sigma, **kw):
    """``judge`` and assert both verdicts."""
    m = judge(got, name, eps, sigma, **kw)
    assert m["ok_element"], m
    assert m["ok_rows"], m
    return m
