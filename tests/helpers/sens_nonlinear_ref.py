"""Long-double references of the seven sensitivity calls (csrc/sens.h) on the NONLINEAR models -- TEST
INFRASTRUCTURE ONLY (tests/test_sens_nonlinear_cpu.py, tests/test_gpu_sens_nonlinear.py).

The glue between two things the suite already has: the exact stage derivatives of helpers/stage_derivs_ref.py
(hyper-dual numbers over np.longdouble: A_k, B_k and H_k = hess(q_k + lam_{k+1}^T F_k), no truncation) and
the restatements of the kernels' two rounds from generic per-stage operands (helpers/sens_ref.py,
sens_p_ref.py, sens_vjp_ref.py, sens_bounds_ref.py, sens_weights_ref.py).  Nothing here reads the kernel:
the conventions are those include/mpcx.h states --

* stage k < N is evaluated at (X_k, U_k) of w, STAGE 0 AT (x0, U_0) with x0 = P[:nx]; the gradient scale is 1;
* stage k's multiplier is lam_g[nx (k + 1) : nx (k + 2)] (g_{k+1} = F(X_k, U_k) - X_{k+1}), with a plus sign;
* the stage row is (x_ref, 0) at every stage under the layout x0_xref and row k of P under x0_stageref (for
  the path-frame bicycle it enters the dynamics);
* Sigma = sens_ref.sigma_of, its one-sided split sens_bounds_ref.split_sigma;
* right-hand sides: sens_p / sens_vjp r_k = G_k dzr_k with G_k = d(grad_z q_k)/d zr_k (the exact mixed
  derivative, one hyper-dual pass with z on e1 and the reference on e2: -2 W for the node costs), d_k = 0,
  gP = (lam~_0, G_k^T z~_k), the x0_xref block the stage sum; weights r_k = grad_z q_k evaluated with the
  direction in the weights' place (q is linear in them: 2 dW_k e_k for the node costs; the path bicycle's
  hook weight w_z is no part of the row); bounds sens_bounds_ref.bound_rhs.

Every ``reference_*`` takes ``dtype``: np.longdouble is the reference (both rounds and the residuals in long
double), np.float64 the same pipeline at the device's precision -- float64 hyper-dual operands, the float64
recursion, residuals in long double rounded to float64, as the kernel's refinement step.  The distance
between the two (``e64``) is what rounding alone does to a call at a point: the yardstick E64(case, call).

Per instance: P_b (n_p,), sol = {"w", "lam_g", "lam_x"} rows of one instance, lb / ub (n_w,) with +-1e20 =
none.  Directions and cotangents are row-major as the Solver's arguments (m, .), results as its outputs.
"""
import numpy as np
import sens_bounds_ref as sb
import sens_p_ref as sp
import sens_ref as sr
import sens_weights_ref as sw
import stage_derivs_ref as sd
from sens_ref import iu_w, ix_w

LD = np.longdouble


# ---------------------------------------------------------------------------------------------------
# the problem's stages
# ---------------------------------------------------------------------------------------------------
def model_of(ocp):
    return getattr(ocp, "model", "unicycle")


def dims(ocp):
    return ocp.nx, ocp.nu, ocp.N


def stage_points(ocp, P_b, w, dtype, stage0=None):
    """(Z (N, nz), zr (N, nz)): the points (X_k, U_k) the stages are evaluated at -- stage 0 at (x0, U_0),
    x0 = P_b[:nx] (``stage0``: another state in its place, for the tests of the reference's own teeth) --
    and the stage rows of P_b's layout."""
    nx, nu, N = dims(ocp)
    nz = nx + nu
    P_b, w = np.asarray(P_b, dtype), np.asarray(w, dtype)
    Z = np.zeros((N, nz), dtype)
    for k in range(N):
        Z[k, :nx], Z[k, nx:] = w[ix_w(nx, nu, k)], w[iu_w(nx, nu, k)]
    Z[0, :nx] = P_b[:nx] if stage0 is None else np.asarray(stage0, dtype)
    if ocp.param == "x0_xref":
        zr = np.zeros((N, nz), dtype)
        zr[:, :nx] = P_b[nx:2 * nx]
    else:
        zr = P_b[nx:].reshape(N, nz).copy()
    return Z, zr


def multipliers(ocp, lam_g, dtype):
    """lam (N, nx): row k = the multiplier of g_{k+1} = F(X_k, U_k) - X_{k+1}"""
    nx, _, N = dims(ocp)
    return np.asarray(lam_g, dtype)[nx:].reshape(N, nx).copy()


def unpack(Hp, nz):
    """(n, nz (nz + 1) / 2) in stage_derivs_ref.symix order -> (n, nz, nz) symmetric"""
    iu = np.triu_indices(nz)
    H = np.zeros((Hp.shape[0], nz, nz), Hp.dtype)
    H[:, iu[0], iu[1]] = Hp
    H[:, iu[1], iu[0]] = Hp
    return H


def operands(ocp, P_b, w, lam_g, dtype=LD, gauss_newton=False, stage0=None):
    """(A (N, nx, nx), B (N, nx, nu), H (N, nz, nz)) per stage in ``dtype``: stage_derivs_ref.stage_derivs at
    ``stage_points`` with ``multipliers`` and fs = 1.  ``gauss_newton`` (H at lam = 0) and ``stage0`` give the
    deliberately wrong variants of tests/test_sens_nonlinear_cpu.py."""
    nx, nu, _ = dims(ocp)
    Z, zr = stage_points(ocp, P_b, w, dtype, stage0)
    lam = multipliers(ocp, lam_g, dtype)
    if gauss_newton:
        lam = np.zeros_like(lam)
    d = sd.stage_derivs(model_of(ocp), Z, lam, zr, 1.0, ocp.T, ocp.M, ocp.Q, ocp.R, getattr(ocp, "par", ()),
                        dtype=dtype, cost=ocp.cost)
    return d["A"], d["B"], unpack(d["H"], nx + nu)


def _stage_args(ocp, dtype, no_hook=False):
    par = [dtype(p) for p in getattr(ocp, "par", ())]
    if no_hook and model_of(ocp) == "path_bicycle":
        par[3] = dtype(0)  # w_z is no part of the weight row
    return model_of(ocp), par, dtype(ocp.T), ocp.M, ocp.cost


def _cost(model, zs, row, W, par, T, M, cost):
    """q alone: only the unicycle's quadrature needs the integrator's stage states"""
    return sd.unicycle_stage(zs, row, W, T, M, cost)[1] if model == "unicycle" else sd.stage_cost(model, zs, row, W, par)


def cost_gradient(ocp, Z, zr, W, dtype=LD, no_hook=False):
    """grad_z q (N, nz) at the points Z with the stage rows zr and the weights W (N, nz) -- one row per
    stage, so that a per-stage direction of the weights can stand in their place -- by hyper-dual numbers."""
    model, par, T, M, cost = _stage_args(ocp, dtype, no_hook)
    Z, zr, W = (np.asarray(v, dtype) for v in (Z, zr, W))
    n, nz = Z.shape
    one, zero = np.ones(n, dtype), np.zeros(n, dtype)
    row, Wl = [zr[:, i] for i in range(nz)], [W[:, i] for i in range(nz)]
    g = np.zeros((n, nz), dtype)
    for a in range(nz):
        zs = [sd.HD(Z[:, i], one if i == a else zero, zero, zero) for i in range(nz)]
        g[:, a] = _cost(model, zs, row, Wl, par, T, M, cost).a + zero
    return g


def cost_mixed(ocp, Z, zr, dtype=LD):
    """G (N, nz, nz), G[k, i, j] = d2 q_k / d z_i d zr_j at the problem's weights: z on e1, the reference on e2.
    Under x0_xref the inputs have no reference: those columns are zero.  Not for the path-frame bicycle (its
    rows enter the dynamics, and sens_p refuses it)."""
    assert model_of(ocp) != "path_bicycle"
    model, par, T, M, cost = _stage_args(ocp, dtype)
    Z, zr = np.asarray(Z, dtype), np.asarray(zr, dtype)
    n, nz = Z.shape
    nref = ocp.nx if ocp.param == "x0_xref" else nz
    one, zero = np.ones(n, dtype), np.zeros(n, dtype)
    W = [dtype(v) + zero for v in list(ocp.Q)[:ocp.nx] + list(ocp.R)[:ocp.nu]]
    G = np.zeros((n, nz, nz), dtype)
    for i in range(nz):
        zs = [sd.HD(Z[:, a], one if a == i else zero, zero, zero) for a in range(nz)]
        for j in range(nref):
            row = [sd.HD(zr[:, a], zero, one if a == j else zero, zero) for a in range(nz)]
            G[:, i, j] = _cost(model, zs, row, W, par, T, M, cost).ab + zero
    return G


# ---------------------------------------------------------------------------------------------------
# one instance's point: operands, Sigma and the factors' verdict, built once and shared by the seven calls
# ---------------------------------------------------------------------------------------------------
class Point:
    def __init__(self, ocp, P_b, sol, lb, ub, dtype=LD, **variant):
        nx, nu, N = dims(ocp)
        self.ocp, self.dtype, self.nx, self.nu, self.N = ocp, dtype, nx, nu, N
        self.P = np.asarray(P_b, dtype)
        self.w = np.asarray(sol["w"], dtype)
        abh = variant.pop("abh", None)  # the operands, where ``points`` has evaluated a whole batch's at once
        self.A, self.B, self.H = operands(ocp, P_b, sol["w"], sol["lam_g"], dtype, **variant) if abh is None else abh
        self.Sig = sr.sigma_of(sol["w"], sol["lam_x"], lb, ub, nx, nu, dtype)
        self.sL, self.sU = sb.split_sigma(sol["w"], sol["lam_x"], lb, ub, nx, dtype)
        self.Z, self.zr = stage_points(ocp, P_b, sol["w"], dtype, variant.get("stage0"))
        self.regular = sp._factors(self.A, self.B, self.H, self.Sig, dtype)[4]
        self._G = None

    @property
    def resid(self):  # the residuals of the refinement round: in long double either way
        return LD

    @property
    def G(self):
        if self._G is None:
            self._G = cost_mixed(self.ocp, self.Z, self.zr, self.dtype)
        return self._G


def points(ocp, P, res, lb, ub, dtype=LD):
    """The Point of every instance of a batch -- P (B, n_p), res a solve's result, lb / ub (n_w,) or (B, n_w) --
    with the stage derivatives of the whole batch from one hyper-dual evaluation."""
    nx, nu, N = dims(ocp)
    B = P.shape[0]
    lb, ub = np.broadcast_to(lb, (B, lb.shape[-1])), np.broadcast_to(ub, (B, ub.shape[-1]))
    ZR = [stage_points(ocp, P[b], res["w"][b], dtype) for b in range(B)]
    lam = np.concatenate([multipliers(ocp, res["lam_g"][b], dtype) for b in range(B)])
    d = sd.stage_derivs(model_of(ocp), np.concatenate([z for z, _ in ZR]), lam, np.concatenate([r for _, r in ZR]), 1.0,
                        ocp.T, ocp.M, ocp.Q, ocp.R, getattr(ocp, "par", ()), dtype=dtype, cost=ocp.cost)
    H = unpack(d["H"], nx + nu)
    return [Point(ocp, P[b], {k: res[k][b] for k in ("w", "lam_g", "lam_x")}, lb[b], ub[b], dtype,
                  abh=tuple(v[b * N:(b + 1) * N] for v in (d["A"], d["B"], H))) for b in range(B)]


def _at(ocp, P_b, sol, lb, ub, dtype, at):
    if at is not None:
        assert at.dtype == dtype
        return at
    return Point(ocp, P_b, sol, lb, ub, dtype)


def two_rounds(pt, rq, rr, x_start):
    """The kernels' two rounds on the Riccati solve of right-hand sides (rq[0..N], rr[0..N-1], d = 0) from
    dX_0 = x_start, as sens_bounds_ref.refined_solve and sens_p_ref.refined_sens_p restate them, with the
    start and the costates kept: (X[0..N], U[0..N-1], lam[0..N]) after the refinement round."""
    A, B, dtype, R = pt.A, pt.B, pt.dtype, lambda v: np.asarray(v, pt.resid)  # noqa: E731
    N, nx = pt.N, pt.nx
    P, K, Huu, Hd, _ = sp._factors(A, B, pt.H, pt.Sig, dtype)
    zero = np.zeros_like(rq[0])
    d = [zero for _ in range(N)]
    X, U, p = sp._sweeps(A, B, P, K, Huu, rq, rr, d, x_start)
    lam = [P[k] @ X[k] + p[k] for k in range(N + 1)]
    eq = [None] * N + [np.asarray(R(P[N]) @ R(X[N]) - R(lam[N]) + R(rq[N]), dtype)]
    er, ed = [None] * N, [None] * N
    for k in range(N):
        eq[k] = np.asarray(R(Hd[k][:nx, :nx]) @ R(X[k]) + R(Hd[k][:nx, nx:]) @ R(U[k]) + R(A[k]).T @ R(lam[k + 1])
                           - R(lam[k]) + R(rq[k]), dtype)
        er[k] = np.asarray(R(Hd[k][nx:, :nx]) @ R(X[k]) + R(Hd[k][nx:, nx:]) @ R(U[k]) + R(B[k]).T @ R(lam[k + 1])
                           + R(rr[k]), dtype)
        ed[k] = np.asarray(R(A[k]) @ R(X[k]) + R(B[k]) @ R(U[k]) - R(X[k + 1]), dtype)
    cX, cU, cp = sp._sweeps(A, B, P, K, Huu, eq, er, ed, zero)
    X = [x + c for x, c in zip(X, cX)]
    U = [u + c for u, c in zip(U, cU)]
    p = [a + c for a, c in zip(p, cp)]
    return X, U, [P[k] @ X[k] + p[k] for k in range(N + 1)]


def _adjoint(pt, gw):
    """(lam~_0 (nx, m), zt (N, nz, m)) of cotangents gw (m, n_w): rq_k = gX_k on every node, rr_k = gU_k, zero start"""
    nx, nu, N = pt.nx, pt.nu, pt.N
    g = np.asarray(gw, pt.dtype).T
    rq = [g[ix_w(nx, nu, k)] for k in range(N + 1)]
    rr = [g[iu_w(nx, nu, k)] for k in range(N)]
    X, U, lam = two_rounds(pt, rq, rr, np.zeros_like(rq[0]))
    return lam[0], np.stack([np.concatenate([X[k], U[k]]) for k in range(N)])


# ---------------------------------------------------------------------------------------------------
# the seven calls
# ---------------------------------------------------------------------------------------------------
def reference_x0(ocp, P_b, sol, lb, ub, dtype=LD, at=None):
    """(dw_dx0 (n_w, nx), regular) of Solver.sens_x0"""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    nx, nu, N = pt.nx, pt.nu, pt.N
    zq, zu = np.zeros((nx, nx), dtype), np.zeros((nu, nx), dtype)
    X, U, _ = two_rounds(pt, [zq] * (N + 1), [zu] * N, np.eye(nx, dtype=dtype))
    return sp._pack(X, U, nx, nu, dtype), pt.regular


def _ref_directions(pt, dP):
    """dzr (N, nz, m) of directions dP (m, n_p) of the parameter row"""
    nx, nu, N = pt.nx, pt.nu, pt.N
    nz, m = nx + nu, dP.shape[0]
    dzr = np.zeros((N, nz, m), pt.dtype)
    if pt.ocp.param == "x0_xref":
        dzr[:, :nx, :] = dP[:, nx:2 * nx].T[None]
    else:
        dzr[:] = np.transpose(dP[:, nx:].reshape(m, N, nz), (1, 2, 0))
    return dzr


def reference_p(ocp, P_b, sol, lb, ub, dP, dtype=LD, at=None):
    """(dw (n_w, m), regular) of Solver.sens_p for the directions dP (m, n_p)"""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    nx, nu, N = pt.nx, pt.nu, pt.N
    dP = np.atleast_2d(np.asarray(dP, dtype))
    r = np.einsum("kij,kjm->kim", pt.G, _ref_directions(pt, dP))
    rq = [r[k][:nx] for k in range(N)] + [np.zeros((nx, dP.shape[0]), dtype)]
    rr = [r[k][nx:] for k in range(N)]
    X, U, _ = two_rounds(pt, rq, rr, dP[:, :nx].T.copy())
    return sp._pack(X, U, nx, nu, dtype), pt.regular


def reference_vjp(ocp, P_b, sol, lb, ub, gw, dtype=LD, at=None):
    """(gP (m, n_p), regular) of Solver.sens_vjp for the cotangents gw (m, n_w)"""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    nx, nu, N = pt.nx, pt.nu, pt.N
    nz = nx + nu
    lam0, zt = _adjoint(pt, np.atleast_2d(gw))
    gzr = np.einsum("kij,kim->kjm", pt.G, zt)  # G_k^T z~_k
    gP = np.zeros((lam0.shape[1], pt.P.size), dtype)
    gP[:, :nx] = lam0.T
    if ocp.param == "x0_xref":
        gP[:, nx:2 * nx] = np.sum(gzr[:, :nx, :], axis=0).T
    else:
        gP[:, nx:] = np.transpose(gzr, (2, 0, 1)).reshape(-1, N * nz)
    return gP, pt.regular


def reference_bounds(ocp, P_b, sol, lb, ub, dlb, dub, dtype=LD, at=None):
    """(dw (n_w, m), regular) of Solver.sens_bounds for the directions dlb, dub (m, n_w)"""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    dlb, dub = np.atleast_2d(np.asarray(dlb, dtype)).T, np.atleast_2d(np.asarray(dub, dtype)).T
    return sb.refined_bounds_sens(pt.A, pt.B, pt.H, pt.sL, pt.sU, dlb, dub, pt.resid, dtype)[1], pt.regular


def reference_bounds_vjp(ocp, P_b, sol, lb, ub, gw, dtype=LD, at=None):
    """(glbw (m, n_w), gubw (m, n_w), regular) of Solver.sens_bounds_vjp for the cotangents gw (m, n_w)"""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    g = np.atleast_2d(np.asarray(gw, dtype)).T
    gl, gu = sb.refined_bounds_vjp(pt.A, pt.B, pt.H, pt.sL, pt.sU, g, pt.resid, dtype)
    return gl.T.copy(), gu.T.copy(), pt.regular


def _weight_rhs(pt, dQ, dR):
    """r (N, nz, m): grad_z q_k with direction c's per-stage row (dQ, dR)[c, k] in the weights' place"""
    d = np.concatenate([np.asarray(dQ, pt.dtype), np.asarray(dR, pt.dtype)], axis=2)  # (m, N, nz)
    m, N, nz = d.shape
    g = cost_gradient(pt.ocp, np.tile(pt.Z, (m, 1)), np.tile(pt.zr, (m, 1)), d.reshape(m * N, nz), pt.dtype, no_hook=True)
    return np.ascontiguousarray(np.transpose(g.reshape(m, N, nz), (1, 2, 0)))


def reference_weights(ocp, P_b, sol, lb, ub, dQ, dR, dtype=LD, at=None):
    """(dw (n_w, m), regular) of Solver.sens_weights for per-stage directions dQ (m, N, nx), dR (m, N, nu)"""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    r = _weight_rhs(pt, dQ, dR)
    return sw.refined_weights_sens(pt.A, pt.B, pt.H, pt.Sig, r, pt.resid, dtype)[1], pt.regular


def reference_weights_vjp(ocp, P_b, sol, lb, ub, gw, dtype=LD, at=None):
    """(gQk (m, N, nx), gRk (m, N, nu), gQ (m, nx), gR (m, nu), regular) of Solver.sens_weights_vjp:
    gWk[c, k, i] = z~_k^T grad_z q_k at the unit weight i, the sums over the stages in ``dtype``."""
    pt = _at(ocp, P_b, sol, lb, ub, dtype, at)
    nx, N, nz = pt.nx, pt.N, pt.nx + pt.nu
    g = np.atleast_2d(np.asarray(gw, dtype)).T
    zt = sw.refined_adjoint_z(pt.A, pt.B, pt.H, pt.Sig, g, pt.resid, dtype)  # (N, nz, m)
    unit = np.repeat(np.eye(nz, dtype=dtype), N, axis=0)  # rows i N .. (i + 1) N: the unit weight i at every stage
    gq = cost_gradient(ocp, np.tile(pt.Z, (nz, 1)), np.tile(pt.zr, (nz, 1)), unit, dtype, no_hook=True).reshape(nz, N, nz)
    gk = np.einsum("kam,ika->mki", zt, gq)
    gs = np.sum(gk, axis=1)
    return gk[..., :nx], gk[..., nx:], gs[:, :nx], gs[:, nx:], pt.regular


# ---------------------------------------------------------------------------------------------------
# the calls by name, their results stacked for entrywise comparison, and the yardstick E64
# ---------------------------------------------------------------------------------------------------
CALLS = ("x0", "p", "vjp", "bounds", "bounds_vjp", "weights", "weights_vjp")
_REFERENCE = {"x0": reference_x0, "p": reference_p, "vjp": reference_vjp, "bounds": reference_bounds,
              "bounds_vjp": reference_bounds_vjp, "weights": reference_weights, "weights_vjp": reference_weights_vjp}


def stacked(call, ocp, P_b, sol, lb, ub, args=(), dtype=LD, at=None):
    """(every output of ``call`` flattened into one vector, regular)"""
    out = _REFERENCE[call](ocp, P_b, sol, lb, ub, *args, dtype=dtype, at=at)
    return np.concatenate([np.ravel(v) for v in out[:-1]]), out[-1]


def linear_yardstick(call):
    """the helpers' yardstick of the linear tests for this call"""
    import sens_vjp_ref as sv

    return {"x0": sr.e_ref, "p": sp.e_ref_p, "vjp": sv.e_ref_vjp, "bounds": sb.e_ref_b, "bounds_vjp": sb.e_ref_bvjp,
            "weights": sw.e_ref_w, "weights_vjp": sw.e_ref_wvjp}[call]()


def e64(call, ocp, P_b, sol, lb, ub, args=(), at=None, at64=None):
    """(E64, reference in long double stacked, regular): sens_ref.rel_err of the float64 pipeline against the
    long-double one for one instance and call"""
    ref, ok = stacked(call, ocp, P_b, sol, lb, ub, args, LD, at)
    f64, _ = stacked(call, ocp, P_b, sol, lb, ub, args, np.float64, at64)
    return sr.rel_err(f64, ref), ref, ok
