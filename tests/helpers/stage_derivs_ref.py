"""Exact stage derivatives of the nonlinear ODE models in extended precision -- TEST INFRASTRUCTURE
ONLY (tests/test_stage_derivs_cpu.py, tests/test_gpu_stage_derivs.py; through helpers/sens_nonlinear_ref.py
tests/test_sens_nonlinear_cpu.py and tests/test_gpu_sens_nonlinear.py).

For the kinematic bicycle, the 6-state dynamic bicycle, the cart-pole and the path-frame bicycle
this module restates, from the equations in ``mpcx/ode.py``'s docstring and ``oracle/ode_ref.py``
(not from the kernel), the interval map F (RK4, M substeps of h = T/M) and the stage cost q -- and for
the unicycle, from ``oracle/nlp_ref.py``, F with either of its costs (RK4 quadrature, node) -- and
differentiates them with hyper-dual numbers v + a e1 + b e2 + ab e1 e2 (e1^2 = e2^2 = 0) over NumPy
arrays: one pass seeded with (e_m, e_n) gives columns m and n of the first derivatives and the
mixed second derivative, exactly (no truncation).  The scalar type is a parameter: ``np.longdouble``
(64-bit mantissa on x86) is the reference, ``np.float64`` the same algorithm at the device's
precision -- the distance between the two (``yardstick``) is what rounding alone does to each
block, and so the unit in which the device's error is measured.

No knowledge of which derivatives vanish goes in: every one of the nz (nz + 1) / 2 pairs is a pass.

The same model functions run on ``mpmath`` numbers (tests/test_stage_derivs_cpu.py checks the
hyper-dual algebra against 50-digit finite differences of them).
"""
from __future__ import annotations

import functools
import math

import numpy as np

MODEL_ID = {"kin_bicycle": 3, "dyn_bicycle": 4, "cartpole": 5, "path_bicycle": 6}  # tests/hip/derivs_check.hip
NXU = {"kin_bicycle": (3, 2), "dyn_bicycle": (6, 2), "cartpole": (4, 1), "path_bicycle": (4, 2), "unicycle": (3, 2)}
# states f never reads (from the equations): their columns of dF/dx are unit vectors
INDEP = {"kin_bicycle": (0, 1), "dyn_bicycle": (0, 1), "cartpole": (0,), "path_bicycle": ()}
BLOCKS = ("xf", "q", "A", "B", "g", "H")


def symix(i, j, n):
    """Packed upper-triangular index of a symmetric n x n matrix (row-major over i <= j)."""
    if i > j:
        i, j = j, i
    return i * n - i * (i - 1) // 2 + (j - i)


# ---------------------------------------------------------------------------- hyper-dual numbers
class HD:
    """v + a e1 + b e2 + ab e1 e2 over arrays (or scalars) of one dtype."""
    __slots__ = ("v", "a", "b", "ab")
    __array_ufunc__ = None  # ndarray (op) HD defers to HD's reflected operators

    def __init__(self, v, a, b, ab):
        self.v, self.a, self.b, self.ab = v, a, b, ab

    def __neg__(self):
        return HD(-self.v, -self.a, -self.b, -self.ab)

    def __add__(self, o):
        if isinstance(o, HD):
            return HD(self.v + o.v, self.a + o.a, self.b + o.b, self.ab + o.ab)
        return HD(self.v + o, self.a, self.b, self.ab)

    __radd__ = __add__

    def __sub__(self, o):
        if isinstance(o, HD):
            return HD(self.v - o.v, self.a - o.a, self.b - o.b, self.ab - o.ab)
        return HD(self.v - o, self.a, self.b, self.ab)

    def __rsub__(self, o):
        return HD(o - self.v, -self.a, -self.b, -self.ab)

    def __mul__(self, o):
        if isinstance(o, HD):
            return HD(self.v * o.v, self.a * o.v + self.v * o.a, self.b * o.v + self.v * o.b,
                      self.ab * o.v + self.a * o.b + self.b * o.a + self.v * o.ab)
        return HD(self.v * o, self.a * o, self.b * o, self.ab * o)

    __rmul__ = __mul__

    def recip(self):
        """1/y: d = -y'/y^2, d2 = -y''/y^2 + 2 y'_a y'_b / y^3."""
        r = 1 / self.v
        r2 = r * r
        return HD(r, -r2 * self.a, -r2 * self.b, -r2 * self.ab + 2 * r2 * r * self.a * self.b)

    def __truediv__(self, o):
        if isinstance(o, HD):
            return self * o.recip()
        return HD(self.v / o, self.a / o, self.b / o, self.ab / o)

    def __rtruediv__(self, o):
        return self.recip() * o

    def sin(self):
        s, c = np.sin(self.v), np.cos(self.v)
        return HD(s, c * self.a, c * self.b, c * self.ab - s * self.a * self.b)

    def cos(self):
        s, c = np.sin(self.v), np.cos(self.v)
        return HD(c, -s * self.a, -s * self.b, -s * self.ab - c * self.a * self.b)

    def tan(self):
        t = np.tan(self.v)
        d = 1 + t * t  # tan' = 1 + tan^2, tan'' = 2 tan tan'
        return HD(t, d * self.a, d * self.b, d * self.ab + 2 * t * d * self.a * self.b)


def _elementary(name):
    def fn(x):
        if isinstance(x, HD):
            return getattr(x, name)()
        if type(x).__module__.split(".")[0] == "mpmath":
            import mpmath

            return getattr(mpmath, name)(x)
        return getattr(np, name)(x)

    return fn


sin, cos, tan = _elementary("sin"), _elementary("cos"), _elementary("tan")


# ---------------------------------------------------------------------------- the four ODE models, the unicycle
# x, u, par, row: sequences of scalars of one arithmetic (HD, ndarray, mpmath); returns the list dx
def f_kin_bicycle(x, u, par, row):
    """x = (X, Y, psi), u = (v, delta): psi' = v tan(delta) / L."""
    psi, v, d = x[2], u[0], u[1]
    return [v * cos(psi), v * sin(psi), v * tan(d) / par[0]]


def f_dyn_bicycle(x, u, par, row):
    """x = (X, Y, psi, vx, vy, r), u = (delta, ax); linear tyres, par = (m, a, b, Ca, Jz)."""
    m, a, b, Ca, Jz = par[:5]
    psi, vx, vy, r = x[2], x[3], x[4], x[5]
    d, ax = u[0], u[1]
    Fyf = 2 * Ca * (d - (vy + a * r) / vx)
    Fyr = 2 * Ca * (-((vy - b * r) / vx))
    sp, cp, sd, cd = sin(psi), cos(psi), sin(d), cos(d)
    return [vx * cp - vy * sp,
            vx * sp + vy * cp,
            r,
            ax + r * vy - Fyf * sd / m,
            (Fyf * cd + Fyr) / m - vx * r,
            (a * Fyf * cd - b * Fyr) / Jz]


def f_cartpole(x, u, par, row):
    """x = (p, p', phi, phi'), u = F; par = (M, m, L, g, c)."""
    Mc, m, L, g, c = par[:5]
    pd, phi, phid, F = x[1], x[2], x[3], u[0]
    s, co = sin(phi), cos(phi)
    pdd = (F - c * pd - m * L * (phid * phid) * s + m * g * (s * co)) / (Mc + m * (s * s))
    return [pd, pdd, phid, (g * s + co * pdd) / L]


def f_path_bicycle(x, u, par, row):
    """The integrated states x = (y, phi, v) with u = (delta, a), delta the held steering;
    row = (yt, phit, vdes, kappa, d_ref, a_ref), par = (L, c1, c2, w_z)."""
    y, phi, v = x[0], x[1], x[2]
    delta, a = u[0], u[1]
    c1, c2 = par[1], par[2]
    yt, phit, kap = row[0], row[1], row[3]
    e = phi - phit
    return [v * sin(e), v * (c2 * tan(c1 * delta) - kap * cos(e) / (1 - (y - yt) * kap)), a]


def f_unicycle(x, u, par, row):
    """x = (x, y, theta), u = (v, omega): oracle/nlp_ref.py ``rhs``."""
    th, v, om = x[2], u[0], u[1]
    return [v * cos(th), v * sin(th), om]


F_OF = {"kin_bicycle": f_kin_bicycle, "dyn_bicycle": f_dyn_bicycle, "cartpole": f_cartpole,
        "path_bicycle": f_path_bicycle, "unicycle": f_unicycle}


def rk4(f, x, u, par, row, h, M):
    for _ in range(M):
        k1 = f(x, u, par, row)
        k2 = f([xi + (h / 2) * ki for xi, ki in zip(x, k1)], u, par, row)
        k3 = f([xi + (h / 2) * ki for xi, ki in zip(x, k2)], u, par, row)
        k4 = f([xi + h * ki for xi, ki in zip(x, k3)], u, par, row)
        x = [xi + (h / 6) * (a + 2 * b + 2 * c + d) for xi, a, b, c, d in zip(x, k1, k2, k3, k4)]
    return x


def interval(model, z, row, par, T, M):
    """The interval map F: z = (x, u) -> x+ (list of nx)."""
    nx = NXU[model][0]
    h = T / M
    if model == "path_bicycle":
        delta = z[3] + z[4]  # the steering s + d, held over the interval; s+ = delta exactly
        return rk4(f_path_bicycle, z[:3], [delta, z[5]], par, row, h, M) + [delta]
    return rk4(F_OF[model], z[:nx], z[nx:], par, row, h, M)


def stage_cost(model, z, row, W, par):
    """sum W_i (z_i - zr_i)^2, and for the path-frame bicycle (slot 3 of its row is the curvature,
    s has the reference 0) + w_z (tan(s + d) - L kappa)^2."""
    q = None
    for i in range(len(z)):
        d = z[i] if (model == "path_bicycle" and i == 3) else z[i] - row[i]
        t = W[i] * (d * d)
        q = t if q is None else q + t
    if model == "path_bicycle":
        r = tan(z[3] + z[4]) - par[0] * row[3]
        q = q + par[3] * (r * r)
    return q


def unicycle_stage(z, row, W, T, M, cost):
    """(x+, q) of the unicycle, restated from oracle/nlp_ref.py ``F`` (``rhs``, ``stage_L``): RK4 with M
    substeps of DT = T / M; cost "quadrature": q = sum over the substeps of DT / 6 (L1 + 2 L2 + 2 L3 + L4)
    with L = sum W_i (z_i - zr_i)^2 at the four RK4 stage states (the input held); cost "node": q = L at
    the node itself."""
    h = T / M
    x, u = list(z[:3]), list(z[3:])
    L = lambda xs: stage_cost("unicycle", list(xs) + u, row, W, None)  # noqa: E731
    q = L(x) if cost == "node" else None
    for _ in range(M):
        k1 = f_unicycle(x, u, None, row)
        x2 = [xi + (h / 2) * ki for xi, ki in zip(x, k1)]
        k2 = f_unicycle(x2, u, None, row)
        x3 = [xi + (h / 2) * ki for xi, ki in zip(x, k2)]
        k3 = f_unicycle(x3, u, None, row)
        x4 = [xi + h * ki for xi, ki in zip(x, k3)]
        k4 = f_unicycle(x4, u, None, row)
        if cost == "quadrature":
            t = (h / 6) * (L(x) + 2 * L(x2) + 2 * L(x3) + L(x4))
            q = t if q is None else q + t
        x = [xi + (h / 6) * (a + 2 * b + 2 * c + d) for xi, a, b, c, d in zip(x, k1, k2, k3, k4)]
    return x, q


def evaluate(model, z, row, W, par, T, M, cost="node"):
    """(x+ (list of nx), q) of one stage in the arithmetic of its arguments; ``cost`` is read by the
    unicycle alone (the ODE models have the node cost)."""
    if model == "unicycle":
        assert cost in ("node", "quadrature")
        return unicycle_stage(z, row, W, T, M, cost)
    return interval(model, z, row, par, T, M), stage_cost(model, z, row, W, par)


# ---------------------------------------------------------------------------- the reference
def stage_derivs(model, Z, lam, zr, fs, T, M, Q, R, par, dtype=np.longdouble, cost="node"):
    """Z (n, nz), lam (n, nx), zr (n, nz) stage rows -> dict of
    xf (n, nx), q (n,) unscaled, A (n, nx, nx), B (n, nx, nu), g = fs grad q (n, nz) and
    H = fs hess q + hess(lam^T F) (n, nz (nz + 1) / 2) packed in ``symix`` order, all in ``dtype``.
    ``cost``: the unicycle's "node" or "quadrature" (``evaluate``)."""
    nx, nu = NXU[model]
    nz = nx + nu
    Z, lam, zr = (np.asarray(v, dtype=dtype) for v in (Z, lam, zr))
    n = Z.shape[0]
    par = [dtype(p) for p in par]
    W = [dtype(w) for w in list(Q)[:nx] + list(R)[:nu]]
    T, fs = dtype(T), dtype(fs)
    zc = [Z[:, i] for i in range(nz)]
    row = [zr[:, i] for i in range(nz)]
    one, zero = np.ones(n, dtype), np.zeros(n, dtype)
    out = {"xf": np.zeros((n, nx), dtype), "q": np.zeros(n, dtype), "g": np.zeros((n, nz), dtype),
           "H": np.zeros((n, nz * (nz + 1) // 2), dtype)}
    J = np.zeros((n, nx, nz), dtype)
    for m in range(nz):
        for nn in range(m, nz):
            zs = [HD(zc[i], one if i == m else zero, one if i == nn else zero, zero) for i in range(nz)]
            xs, qs = evaluate(model, zs, row, W, par, T, M, cost)
            h = fs * qs.ab
            for r in range(nx):
                h = h + lam[:, r] * xs[r].ab
            out["H"][:, symix(m, nn, nz)] = h
            if nn == m:
                out["g"][:, m] = fs * qs.a
                for r in range(nx):
                    J[:, r, m] = xs[r].a
                if m == 0:
                    out["q"] = qs.v + zero
                    for r in range(nx):
                        out["xf"][:, r] = xs[r].v
    out["A"], out["B"] = J[:, :, :nx].copy(), J[:, :, nx:].copy()
    return out


def split_flat(model, flat):
    """The harness's per-point output (xf, q, A, B, g, H) as a dict of blocks (n, size)."""
    nx, nu = NXU[model]
    nz = nx + nu
    sizes = (nx, 1, nx * nx, nx * nu, nz, nz * (nz + 1) // 2)
    out, o = {}, 0
    for name, s in zip(BLOCKS, sizes):
        out[name] = flat[:, o:o + s]
        o += s
    assert o == flat.shape[1]
    return out


def n_out(model):
    nx, nu = NXU[model]
    nz = nx + nu
    return nx + 1 + nx * nx + nx * nu + nz + nz * (nz + 1) // 2


def block_errors(got, ref, blocks=BLOCKS):
    """Per block: the worst over the points of max |got - ref| / max |ref| (each point's largest
    entry of the block), evaluated in the reference's precision."""
    err = {}
    for name in blocks:
        r = np.asarray(ref[name])
        r = r.reshape(r.shape[0], -1)
        g = np.asarray(got[name]).reshape(r.shape).astype(r.dtype)
        scale = np.max(np.abs(r), axis=1)
        assert np.all(scale > 0), name
        err[name] = float(np.max(np.max(np.abs(g - r), axis=1) / scale))
    return err


# ---------------------------------------------------------------------------- cases of the tests
@functools.lru_cache(maxsize=None)
def constants(model, steer="bicycle"):
    """(T, default M, Q, R, par).  T, M and par are the builders' of ``mpcx.ode``; the weights are the
    tests' own, every one non-zero so that each reference of the cost shows in q and g."""
    from mpcx import ode

    if model == "kin_bicycle":
        o = ode.kinematic_bicycle_tracking()
        return o.T, o.M, (1.0, 1.3, 0.1), (0.5, 0.05), tuple(o.par)
    if model == "dyn_bicycle":
        o = ode.dynamic_bicycle_lane_change()
        return o.T, o.M, (1.0, 0.7, 2.0, 0.3, 1.1, 0.9), (1.0, 0.2), tuple(o.par)
    if model == "cartpole":
        o = ode.cartpole_swingup()
        return o.T, o.M, (1.44, 0.03, 1.0, 0.02), (1e-4,), tuple(o.par)
    o = ode.path_bicycle_lane_keeping(L=3.5, steer=steer)
    return o.T, o.M, (1.75 / 21, 2.5 / 21, 2.5 / 21, 0.3 / 21), (0.2 / 21, 0.4 / 21), tuple(o.par)


N_POINTS = 256  # four waves


@functools.lru_cache(maxsize=None)
def points(model, n=N_POINTS):
    """Seeded random points (Z, lam, zr) of the model's domain; lam = N(0, 1) 10^U(-2, 2) per point."""
    nx, nu = NXU[model]
    rng = np.random.default_rng(1000 + MODEL_ID[model])
    U = lambda lo, hi: rng.uniform(lo, hi, n)  # noqa: E731
    pi = math.pi
    if model == "kin_bicycle":  # delta beyond the +-pi/4 box, so that tan'' matters
        Z = np.stack([U(-2, 2), U(-2, 2), U(-pi, pi), U(-1.5, 1.5), U(-1.2, 1.2)], axis=1)
        zr = Z + rng.normal(0, 0.3, Z.shape)
    elif model == "dyn_bicycle":  # the box of tests/test_gpu_ode.py's adjoint-vs-passes test
        Z = np.stack([U(-50, 50), U(-5, 5), U(-pi, pi), U(2.5, 30.0), U(-2, 2), U(-1, 1), U(-0.5, 0.5), U(-5, 5)], axis=1)
        zr = Z + rng.normal(0, 1, Z.shape)
    elif model == "cartpole":  # swing-up magnitudes
        Z = np.stack([U(-2, 2), U(-3, 3), U(-pi, pi), U(-10, 10), U(-200, 200)], axis=1)
        zr = Z + rng.normal(0, 1, Z.shape) * np.array([1, 1, 1, 3, 30.0])
    else:
        yt, phit, vdes, kap = U(-5, 5), U(-pi, pi), U(0, 30), U(-0.1, 0.1)
        delta, s = U(-0.6, 0.6), U(-0.384, 0.384)
        Z = np.stack([yt + U(-3, 3), phit + U(-1, 1), U(0, 30), s, delta - s, U(-2, 2)], axis=1)
        zr = np.stack([yt, phit, vdes, kap, U(-0.1, 0.1), U(-2, 2)], axis=1)
    lam = rng.normal(size=(n, nx)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    for a in (Z, lam, zr):
        a.setflags(write=False)
    return Z, lam, zr


# (id, model, M, use_cache, which, steer): the smallest M that reaches each path of ode.h
CASES = (
    ("kin-M1-cached", "kin_bicycle", 1, 1, 0, "bicycle"),
    ("kin-M3-direct", "kin_bicycle", 3, 1, 0, "bicycle"),
    ("cart-M1-cached", "cartpole", 1, 1, 0, "bicycle"),
    ("cart-M2-direct", "cartpole", 2, 1, 0, "bicycle"),
    ("dyn-M4-adjoint", "dyn_bicycle", 4, 1, 0, "bicycle"),
    ("dyn-M4-passes-cached", "dyn_bicycle", 4, 1, 1, "bicycle"),
    ("dyn-M5-direct", "dyn_bicycle", 5, 1, 0, "bicycle"),
    ("dyn-M1-adjoint", "dyn_bicycle", 1, 1, 0, "bicycle"),
    ("path-M1-cached", "path_bicycle", 1, 1, 0, "bicycle"),
    ("path-M1-cached-as_written", "path_bicycle", 1, 1, 0, "as_written"),
    ("path-M2-direct", "path_bicycle", 2, 1, 0, "bicycle"),
    ("kin-M1-nocache", "kin_bicycle", 1, 0, 0, "bicycle"),
    ("cart-M1-nocache", "cartpole", 1, 0, 0, "bicycle"),
    ("dyn-M4-nocache", "dyn_bicycle", 4, 0, 0, "bicycle"),
    ("path-M1-nocache", "path_bicycle", 1, 0, 0, "bicycle"),
)
FS = (1.0, 0.37)  # 0.37 stands for the solve kernel's gradient scaling 100 / gm


def grid():
    """Every (case, fs, p_layout, k) of the GPU test, with its pytest id."""
    out = []
    for case in CASES:
        for fs in FS:
            layouts = [(1, 0), (1, 3)] if case[1] == "path_bicycle" else [(0, 0), (1, 0), (1, 3)]
            for lay, k in layouts:
                out.append((case, fs, lay, k, f"{case[0]}-fs{fs}-layout{lay}-k{k}"))
    return out


def stage_rows(model, p_layout):
    """The stage row each point's derivatives see: under p_layout 0 (x0, x_ref) the inputs have no reference."""
    zr = points(model)[2]
    if p_layout == 0:
        zr = zr.copy()
        zr[:, NXU[model][0]:] = 0.0
    return zr


@functools.lru_cache(maxsize=None)
def reference(model, M, steer, fs, p_layout, dtype_name="longdouble"):
    """The reference of one case in ``dtype`` (shared by the tests; treat as read-only)."""
    T, _, Q, R, par = constants(model, steer)
    Z, lam, _ = points(model)
    return stage_derivs(model, Z, lam, stage_rows(model, p_layout), fs, T, M, Q, R, par, dtype=getattr(np, dtype_name))


@functools.lru_cache(maxsize=None)
def yardstick(model, M, steer, fs, p_layout):
    """E64 per block: the reference's own algorithm in float64 against its long-double run."""
    return block_errors(reference(model, M, steer, fs, p_layout, "float64"), reference(model, M, steer, fs, p_layout))
