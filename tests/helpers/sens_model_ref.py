"""Long-double references of the sensitivities of the MPC solution to the model (the kernels csrc/sens.h
sens_mdl_kernel and sens_mdl_vjp_kernel) -- TEST INFRASTRUCTURE ONLY (tests/test_sens_model_cpu.py,
tests/test_gpu_sens_model.py).  Nothing here reads the kernel: the conventions are those include/mpcx.h states.

The system is that of helpers/sens_p_ref.py with both right-hand sides,
    (H_k + Sigma_k) dz_k + [A_k B_k]^T lam_{k+1} - [lam_k; 0] + r_k = 0,   Sigma_x dX_N - lam_N = 0,
    A_k dX_k + B_k dU_k + d_k - dX_{k+1} = 0,   dX_0 = 0,
and a model row th_k of stage k (the leading constants of ``par`` of an ODE model, or the stage's tables
(A row-major, B row-major, c) of a linear one) gives, with the multiplier lam_{k+1} of the stage's defect held,
    r_k = G_k dth_k,   G_k[i, j] = d2 (q_k + lam_{k+1}^T F_k) / dz_i dth_j,
    d_k = D_k dth_k,   D_k[r, j] = dF_{k,r} / dth_j.
ODE models: G and D by hyper-dual numbers (helpers/stage_derivs_ref.py: its model functions take ``par`` in
the arithmetic of their arguments) with z on e1 and the constant on e2, the cost hook of the path-frame
bicycle on the same numbers.  Linear models, closed form: d_k = dA_k x_k + dB_k u_k + dc_k,
r_k = (dA_k^T lam_{k+1}; dB_k^T lam_{k+1}).  Stage 0 is evaluated at (x0, U_0), x0 = P[:nx].

The reverse mode: with (z~, lam~) the adjoint solve for a cotangent g (rq_k = gX_k on every node, rr_k = gU_k,
d = 0, zero start) and lam~_k = P_k X~_k + p~_k, <g, dw> = sum_k (z~_k^T r_k + lam~_{k+1}^T d_k), so
    gth_k = G_k^T z~_k + D_k^T lam~_{k+1}.

``solve_rounds`` restates the kernels' two rounds (each: the residuals of the full system, d included, in
``resid`` precision, then their Riccati solve with sens_p_ref's factors and sweeps) from a zero start.  Every
``reference_*`` takes ``dtype``: np.longdouble is the reference, np.float64 the same pipeline at the device's
precision (residuals in long double rounded to float64).  ``e64`` is the distance between the two: the
yardstick E64(case, call).

Layouts: directions dth (m, N, n_th) per stage; G (N, nz, n_th), D (N, nx, n_th); dw (n_w, m); gradient rows
gthk (m, N, n_th), their stage sum gth (m, n_th); cotangents gw (m, n_w).
"""
import numpy as np
import sens_nonlinear_ref as sn
import sens_p_ref as sp
import sens_ref as sr
import stage_derivs_ref as sd
from sens_ref import iu_w, ix_w

LD = np.longdouble
N_TH = {"kin_bicycle": 1, "dyn_bicycle": 5, "cartpole": 5, "path_bicycle": 4}  # include/mpcx.h, mpcx_model_dims
PAR_NAMES = {"kin_bicycle": ("L",), "dyn_bicycle": ("m", "a", "b", "Ca", "Jz"), "cartpole": ("M", "m", "L", "g", "c"),
             "path_bicycle": ("L", "c1", "c2", "w_z")}


def n_th_of(ocp):
    if sn.model_of(ocp) == "linear":
        return ocp.nx * ocp.nx + ocp.nx * ocp.nu + ocp.nx
    return N_TH[sn.model_of(ocp)]


# ---------------------------------------------------------------------------------------------------
# the tangent matrices
# ---------------------------------------------------------------------------------------------------
def ode_tangent(ocp, Z, zr, lam, dtype=LD, drop_mixed=False, drop_defect=False):
    """(G (N, nz, n_th), D (N, nx, n_th)) of an ODE model at the stage points Z (N, nz) with the stage rows zr and
    the multipliers lam (N, nx): n_th nz hyper-dual passes, z_i on e1 and par_j on e2.  ``drop_mixed`` /
    ``drop_defect`` return zeros in place of G / D: the deliberately wrong variants of the teeth tests."""
    model = sn.model_of(ocp)
    nx, nu, N = sn.dims(ocp)
    nz, n_th = nx + nu, N_TH[model]
    Z, zr, lam = (np.asarray(v, dtype) for v in (Z, zr, lam))
    n = Z.shape[0]
    one, zero = np.ones(n, dtype), np.zeros(n, dtype)
    par = [dtype(p) for p in ocp.par]
    W = [dtype(v) + zero for v in list(ocp.Q)[:nx] + list(ocp.R)[:nu]]
    row = [zr[:, i] for i in range(nz)]
    T = dtype(ocp.T)
    G, D = np.zeros((n, nz, n_th), dtype), np.zeros((n, nx, n_th), dtype)
    for j in range(n_th):
        ps = [sd.HD(par[a] + zero, zero, one if a == j else zero, zero) for a in range(len(par))]
        for i in range(nz):
            zs = [sd.HD(Z[:, a], one if a == i else zero, zero, zero) for a in range(nz)]
            xs = sd.interval(model, zs, row, ps, T, ocp.M)
            q = sd.stage_cost(model, zs, row, W, ps)
            mixed = q.ab + zero
            for r in range(nx):
                mixed = mixed + lam[:, r] * xs[r].ab
                if i == 0:
                    D[:, r, j] = xs[r].b + zero
            G[:, i, j] = mixed
    if drop_mixed:
        G = np.zeros_like(G)
    if drop_defect:
        D = np.zeros_like(D)
    return G, D


def linear_rhs(nx, nu, Z, lam, dth, dtype=LD):
    """(r (N, nz, m), d (N, nx, m)) of a linear model's table directions dth (m, N, nx nx + nx nu + nx) in closed
    form at the stage points Z (N, nz) and multipliers lam (N, nx)"""
    Z, lam, dth = (np.asarray(v, dtype) for v in (Z, lam, dth))
    m, N = dth.shape[:2]
    dA = dth[..., :nx * nx].reshape(m, N, nx, nx)
    dB = dth[..., nx * nx:nx * nx + nx * nu].reshape(m, N, nx, nu)
    dc = dth[..., nx * nx + nx * nu:]
    d = np.einsum("ckij,kj->kic", dA, Z[:, :nx]) + np.einsum("ckij,kj->kic", dB, Z[:, nx:]) + np.transpose(dc, (1, 2, 0))
    r = np.concatenate([np.einsum("ckji,kj->kic", dA, lam), np.einsum("ckji,kj->kic", dB, lam)], axis=1)
    return np.ascontiguousarray(r), np.ascontiguousarray(d)


def linear_cotangent(nx, nu, Z, lam, zt, lt):
    """gthk (m, N, n_th) of a linear model: gA_k = lam~_{k+1} x_k^T + lam_{k+1} X~_k^T, gB_k likewise on the inputs,
    gc_k = lam~_{k+1}; zt (N, nz, m) the adjoint solution, lt (N, nx, m) the next node's adjoint costate"""
    gA = np.einsum("krc,km->ckrm", lt, Z[:, :nx]) + np.einsum("kr,kmc->ckrm", lam, zt[:, :nx])
    gB = np.einsum("krc,km->ckrm", lt, Z[:, nx:]) + np.einsum("kr,kmc->ckrm", lam, zt[:, nx:])
    m, N = gA.shape[:2]
    return np.concatenate([gA.reshape(m, N, -1), gB.reshape(m, N, -1), np.transpose(lt, (2, 0, 1))], axis=2)


# ---------------------------------------------------------------------------------------------------
# the kernels' two rounds with both right-hand sides
# ---------------------------------------------------------------------------------------------------
def solve_rounds(A, B, H, Sig, rq, rr, d, dtype=LD, resid=LD, rounds=2):
    """(X[0..N], U[0..N-1], lam[0..N], regular): ``rounds`` rounds from a zero start on the right-hand sides
    rq[0..N] (nx, m), rr[0..N-1] (nu, m), d[0..N-1] (nx, m) -- each round the residuals of the three block rows at
    the current (X, U, lam = P X + p) in ``resid`` rounded to ``dtype``, and their Riccati solve (sens_p_ref's
    factors and sweeps, in ``dtype``) added on.  The first round's residuals are the right-hand sides themselves."""
    A, B, H, Sig = (np.asarray(v, dtype) for v in (A, B, H, Sig))
    rq, rr, d = ([np.asarray(v, dtype) for v in seq] for seq in (rq, rr, d))
    N, nx = A.shape[0], A.shape[1]
    P, K, Huu, Hd, regular = sp._factors(A, B, H, Sig, dtype)
    R = lambda v: np.asarray(v, resid)  # noqa: E731
    zero = np.zeros_like(rq[0])
    X, U, p = [zero] * (N + 1), [np.zeros_like(rr[0])] * N, [zero] * (N + 1)
    for _ in range(rounds):
        lam = [P[k] @ X[k] + p[k] for k in range(N + 1)]
        eq = [None] * N + [np.asarray(R(P[N]) @ R(X[N]) - R(lam[N]) + R(rq[N]), dtype)]
        er, ed = [None] * N, [None] * N
        for k in range(N):
            eq[k] = np.asarray(R(Hd[k][:nx, :nx]) @ R(X[k]) + R(Hd[k][:nx, nx:]) @ R(U[k]) + R(A[k]).T @ R(lam[k + 1])
                               - R(lam[k]) + R(rq[k]), dtype)
            er[k] = np.asarray(R(Hd[k][nx:, :nx]) @ R(X[k]) + R(Hd[k][nx:, nx:]) @ R(U[k]) + R(B[k]).T @ R(lam[k + 1])
                               + R(rr[k]), dtype)
            ed[k] = np.asarray(R(A[k]) @ R(X[k]) + R(B[k]) @ R(U[k]) + R(d[k]) - R(X[k + 1]), dtype)
        cX, cU, cp = sp._sweeps(A, B, P, K, Huu, eq, er, ed, zero)
        X = [x + c for x, c in zip(X, cX)]
        U = [u + c for u, c in zip(U, cU)]
        p = [a + c for a, c in zip(p, cp)]
    return X, U, [P[k] @ X[k] + p[k] for k in range(N + 1)], regular


def forward(A, B, H, Sig, r, d, dtype=LD, rounds=2):
    """(dw (n_w, m), regular) of right-hand sides r (N, nz, m), d (N, nx, m)"""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    r, d = np.asarray(r, dtype), np.asarray(d, dtype)
    rq = [r[k][:nx] for k in range(N)] + [np.zeros((nx, r.shape[2]), dtype)]
    X, U, _, ok = solve_rounds(A, B, H, Sig, rq, [r[k][nx:] for k in range(N)], [d[k] for k in range(N)], dtype, LD, rounds)
    return sp._pack(X, U, nx, nu, dtype), ok


def adjoint(A, B, H, Sig, gw, dtype=LD):
    """(zt (N, nz, m), lt (N, nx, m) = lam~_{k+1}, regular) of cotangents gw (m, n_w)"""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    g = np.asarray(np.atleast_2d(gw), dtype).T
    rq = [g[ix_w(nx, nu, k)] for k in range(N + 1)]
    rr = [g[iu_w(nx, nu, k)] for k in range(N)]
    X, U, lam, ok = solve_rounds(A, B, H, Sig, rq, rr, [np.zeros_like(rq[0])] * N, dtype, LD)
    return np.stack([np.concatenate([X[k], U[k]]) for k in range(N)]), np.stack(lam[1:]), ok


# ---------------------------------------------------------------------------------------------------
# one instance of an ODE case (a sens_nonlinear_ref.Point) or of a linear case (its tables)
# ---------------------------------------------------------------------------------------------------
class LinearPoint:
    """What the references need of one instance of a LinearOCP at a solve's point, in ``dtype``"""

    def __init__(self, lin, P_b, sol, lb, ub, b=0, dtype=LD):
        nx, nu, N = lin.nx, lin.nu, lin.N
        self.ocp, self.dtype, self.nx, self.nu, self.N = lin, dtype, nx, nu, N
        A, Bm, H = sr.linear_operands(lin, b)
        self.A, self.B, self.H = (np.asarray(v, dtype) for v in (A, Bm, H))
        self.Sig = sr.sigma_of(sol["w"], sol["lam_x"], lb, ub, nx, nu, dtype)
        w, P_b = np.asarray(sol["w"], dtype), np.asarray(P_b, dtype)
        self.Z = np.stack([np.concatenate([P_b[:nx] if k == 0 else w[ix_w(nx, nu, k)], w[iu_w(nx, nu, k)]]) for k in range(N)])
        self.lam = np.asarray(sol["lam_g"], dtype)[nx:].reshape(N, nx)


def _ode_lam(pt, sol):
    return sn.multipliers(pt.ocp, sol["lam_g"], pt.dtype)


def reference_model(pt, sol, dth, **variant):
    """(dw (n_w, m), regular) of Solver.sens_model for per-stage directions dth (m, N, n_th) at the point ``pt`` (a
    sens_nonlinear_ref.Point or a LinearPoint, whose dtype is the pipeline's)"""
    dtype = pt.dtype
    dth = np.asarray(dth, dtype)
    if isinstance(pt, LinearPoint):
        r, d = linear_rhs(pt.nx, pt.nu, pt.Z, pt.lam, dth, dtype)
        if variant.get("drop_mixed"):
            r = np.zeros_like(r)
        if variant.get("drop_defect"):
            d = np.zeros_like(d)
    else:
        G, D = ode_tangent(pt.ocp, pt.Z, pt.zr, _ode_lam(pt, sol), dtype, **variant)
        r, d = np.einsum("kij,ckj->kic", G, dth), np.einsum("kij,ckj->kic", D, dth)
    return forward(pt.A, pt.B, pt.H, pt.Sig, r, d, dtype)


def reference_model_vjp(pt, sol, gw):
    """(gthk (m, N, n_th), gth (m, n_th), regular) of Solver.sens_model_vjp for the cotangents gw (m, n_w)"""
    dtype = pt.dtype
    zt, lt, ok = adjoint(pt.A, pt.B, pt.H, pt.Sig, gw, dtype)
    if isinstance(pt, LinearPoint):
        gk = linear_cotangent(pt.nx, pt.nu, pt.Z, pt.lam, zt, lt)
    else:
        G, D = ode_tangent(pt.ocp, pt.Z, pt.zr, _ode_lam(pt, sol), dtype)
        gk = np.einsum("kij,kic->ckj", G, zt) + np.einsum("kij,kic->ckj", D, lt)
    return gk, np.sum(gk, axis=1), ok


def stacked(call, pt, sol, arg):
    if call == "model":
        out = reference_model(pt, sol, arg)
    else:
        out = reference_model_vjp(pt, sol, arg)
    return np.concatenate([np.ravel(v) for v in out[:-1]]), out[-1]


def e64(call, pt, pt64, sol, arg):
    """(E64, the long-double reference stacked, regular): sens_ref.rel_err of the float64 pipeline against the
    long-double one for one instance and call ("model" or "model_vjp")"""
    ref, ok = stacked(call, pt, sol, arg)
    f64, _ = stacked(call, pt64, sol, arg)
    return sr.rel_err(f64, ref), ref, ok


# ---------------------------------------------------------------------------------------------------
# the directions of the tests
# ---------------------------------------------------------------------------------------------------
def relative_directions(ocp, m, seed, per_stage=True):
    """(m, N, n_th) seeded normal directions relative to each constant's size (ODE models: xi |par_j|; linear
    models: xi max(|entry of the instance-0 stage table|, 0.1 max|table|), so a structural zero of a table moves
    too).  per_stage=False: the same row at every stage."""
    N, n_th = ocp.N, n_th_of(ocp)
    rng = np.random.default_rng(seed)
    xi = rng.normal(size=(m, N if per_stage else 1, n_th))
    if sn.model_of(ocp) == "linear":
        tab = np.asarray(ocp.tab)
        tab = tab if tab.ndim == 1 else tab[0]
        c = np.zeros((np.asarray(ocp.A).shape[0], ocp.nx)) if ocp.c is None else np.asarray(ocp.c)
        rows = np.concatenate([np.asarray(ocp.A)[tab].reshape(N, -1), np.asarray(ocp.B)[tab].reshape(N, -1), c[tab]], axis=1)
        size = np.maximum(np.abs(rows), 0.1 * np.max(np.abs(rows)))
        size = size if per_stage else size[:1]
    else:
        size = np.abs(np.array(ocp.par, float))[None, :n_th]
    d = xi * size[None]
    return np.ascontiguousarray(np.broadcast_to(d, (m, N, n_th)))
