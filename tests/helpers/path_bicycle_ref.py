"""NumPy reference of the path-frame kinematic bicycle MPC (model 7, ``mpcx.ode`` "path_bicycle")
-- TEST INFRASTRUCTURE ONLY.  Written from the equations of the model's description, independently
of the kernel:

    x = (y, phi, v, s), u = (d, a); delta = s + d held over the interval
    y'   = v sin(phi - phit)
    phi' = v (c2 tan(c1 delta) - kappa cos(phi - phit) / (1 - (y - yt) kappa))
    v'   = a                                  RK4, M substeps over (y, phi, v)
    s+   = s + d                              exactly
    l    = sum Q_i (x_i - xr_i)^2 + sum R_j (u_j - ur_j)^2 + w_z (tan(delta) - L kappa)^2
    row  = (yt, phit, vdes, kappa, d_ref, a_ref),  (xr, ur) = (yt, phit, vdes, 0, d_ref, a_ref)
    par  = (L, c1, c2, w_z)

PARITY UNPINNED: ``Trajectory Tracking/test2.py`` writes no output file.  Derivatives are complex
steps (exact to rounding); the KKT residual follows ``oracle/ode_ref.Problem.kkt_residual``
(CasADi's convention grad f + J_g^T lam_g + lam_x = 0; interval 0 integrates from the parameter
x0, so X_0 enters only g_0) and adds the bound multipliers' tests.
"""
from __future__ import annotations

import numpy as np

NX, NU, NZ = 4, 2, 6
BIG = 1e19


class PathProblem:
    """The NLP of an ``mpcx.ode.OdeOCP`` with model "path_bicycle" (duck-typed)."""

    def __init__(self, ocp):
        self.N, self.T, self.M = int(ocp.N), float(ocp.T), int(ocp.M)
        self.W = np.array(list(ocp.Q) + list(ocp.R), float)
        self.L, self.c1, self.c2, self.wz = (float(v) for v in ocp.par)
        inf = np.inf
        self.z_lb = np.array([v if np.isfinite(v) else -inf for v in list(ocp.x_lb) + list(ocp.u_lb)], float)
        self.z_ub = np.array([v if np.isfinite(v) else inf for v in list(ocp.x_ub) + list(ocp.u_ub)], float)
        self.z_lb[np.abs(self.z_lb) >= BIG] = -inf
        self.z_ub[np.abs(self.z_ub) >= BIG] = inf

    # ------------------------------------------------------------------ model
    def f(self, xp, delta, a, row):
        """Continuous dynamics of the physical states xp (..., 3) (complex-safe)."""
        y, phi, v = xp[..., 0], xp[..., 1], xp[..., 2]
        yt, phit, kap = row[..., 0], row[..., 1], row[..., 3]
        e = phi - phit
        return np.stack([v * np.sin(e),
                         v * (self.c2 * np.tan(self.c1 * delta) - kap * np.cos(e) / (1.0 - (y - yt) * kap)),
                         a + 0 * v], axis=-1)

    def F(self, z, row):
        """The interval map: z (..., 6) = (x, u) -> x+ (..., 4)."""
        xp, s, d, a = z[..., 0:3], z[..., 3], z[..., 4], z[..., 5]
        delta = s + d
        h = self.T / self.M
        for _ in range(self.M):
            k1 = self.f(xp, delta, a, row)
            k2 = self.f(xp + 0.5 * h * k1, delta, a, row)
            k3 = self.f(xp + 0.5 * h * k2, delta, a, row)
            k4 = self.f(xp + h * k3, delta, a, row)
            xp = xp + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        return np.concatenate([xp, delta[..., None]], axis=-1)

    def l(self, z, row):
        """The full stage cost."""
        ref = np.array(row, dtype=float, copy=True)
        ref[..., 3] = 0.0
        d = z - ref
        r = np.tan(z[..., 3] + z[..., 4]) - self.L * row[..., 3]
        return np.sum(self.W * d * d, axis=-1) + self.wz * r * r

    def jac(self, z, row):
        """dF/dz (..., 4, 6) by complex step."""
        h = 1e-30
        zc = z[..., None, :] + 1j * h * np.eye(NZ)
        Fc = self.F(zc, np.asarray(row)[..., None, :])
        return np.swapaxes(Fc.imag / h, -1, -2)

    def grad_l(self, z, row):
        """dl/dz (..., 6) by complex step."""
        h = 1e-30
        zc = z[..., None, :] + 1j * h * np.eye(NZ)
        return self.l(zc, np.asarray(row)[..., None, :]).imag / h

    # ------------------------------------------------------------------ layout
    def rows(self, P):
        return np.asarray(P, float)[NX:].reshape(self.N, NZ)

    def split_w(self, w):
        w = np.asarray(w, float)
        N = self.N
        X = np.empty((N + 1, NX))
        U = np.empty((N, NU))
        X[0] = w[:NX]
        for k in range(N):
            U[k] = w[NX + NZ * k: NX + NZ * k + NU]
            X[k + 1] = w[NX + NZ * k + NU: NX + NZ * (k + 1)]
        return X, U

    def join_w(self, X, U):
        return np.concatenate([X[0]] + [np.concatenate([U[k], X[k + 1]]) for k in range(self.N)])

    def bounds_w(self):
        """(lbw, ubw): X_0 free, the boxes on (U_k, X_{k+1})."""
        lb = np.concatenate([np.full(NX, -np.inf)] + [np.concatenate([self.z_lb[NX:], self.z_lb[:NX]])] * self.N)
        ub = np.concatenate([np.full(NX, np.inf)] + [np.concatenate([self.z_ub[NX:], self.z_ub[:NX]])] * self.N)
        return lb, ub

    # ------------------------------------------------------------------ single shooting
    def rollout(self, U, x0, rows):
        X = [np.asarray(x0, float)]
        for k in range(self.N):
            X.append(self.F(np.concatenate([X[-1], U[k]]), rows[k]))
        return np.array(X)

    def cost(self, U, P):
        P = np.asarray(P, float)
        rows = self.rows(P)
        U = np.asarray(U, float).reshape(self.N, NU)
        X = self.rollout(U, P[:NX], rows)
        return float(np.sum(self.l(np.concatenate([X[:-1], U], axis=1), rows))), X

    def cost_grad(self, U, P):
        """J(U) and dJ/dU (N, 2) by the adjoint recursion over complex-step Jacobians."""
        P = np.asarray(P, float)
        rows = self.rows(P)
        U = np.asarray(U, float).reshape(self.N, NU)
        X = self.rollout(U, P[:NX], rows)
        Z = np.concatenate([X[:-1], U], axis=1)
        J = float(np.sum(self.l(Z, rows)))
        Jac, gl = self.jac(Z, rows), self.grad_l(Z, rows)
        lam = np.zeros(NX)
        g = np.zeros((self.N, NU))
        for k in range(self.N - 1, -1, -1):
            g[k] = gl[k, NX:] + Jac[k, :, NX:].T @ lam
            lam = gl[k, :NX] + Jac[k, :, :NX].T @ lam
        return J, g

    def solve_slsqp(self, P, U0):
        """The helper's own optimum of the single-shooting form, started at U0 (scipy SLSQP): the
        boxes on (d, a) as bounds, the steering box as linear inequalities on s_0 + cumsum(d)."""
        from scipy.optimize import minimize

        P = np.asarray(P, float)
        N = self.N
        s0 = P[3]
        lo, hi = self.z_lb, self.z_ub
        bnds = [(None if not np.isfinite(lo[NX + j]) else lo[NX + j], None if not np.isfinite(hi[NX + j]) else hi[NX + j])
                for _ in range(N) for j in range(NU)]
        C = np.zeros((N, NU * N))  # s_{k+1} = s0 + C[k] u
        for k in range(N):
            C[k, 0:NU * (k + 1):NU] = 1.0
        cons = []
        if np.isfinite(hi[3]):
            cons.append({"type": "ineq", "fun": lambda u: hi[3] - s0 - C @ u, "jac": lambda u: -C})
        if np.isfinite(lo[3]):
            cons.append({"type": "ineq", "fun": lambda u: s0 + C @ u - lo[3], "jac": lambda u: C})
        sc = 1.0 / max(self.cost(U0, P)[0], 1e-12)  # objective scaled to O(1) for SLSQP's tests

        def fun(u):
            J, g = self.cost_grad(u, P)
            return sc * J, sc * g.reshape(-1)

        r = minimize(fun, np.asarray(U0, float).reshape(-1), jac=True, method="SLSQP", bounds=bnds, constraints=cons,
                     options={"ftol": 1e-15, "maxiter": 400})
        U = r.x.reshape(N, NU)
        J, X = self.cost(U, P)
        return U, X, J, r

    # ------------------------------------------------------------------ multiple shooting
    def kkt(self, w, lam_g, lam_x, P):
        """Certificate of a multiple-shooting primal-dual point.  Returns a dict:
        stat   max |grad f + J_g^T lam_g + lam_x|
        feas   max |g|
        bound  the largest bound violation of w
        sign   the largest wrong-signed part of lam_x (lam_x = z_U - z_L: >= 0 only at an upper
               bound, <= 0 only at a lower one, 0 for a free variable)
        compl  max |lam_x| * (distance to the bound its sign names)
        """
        P = np.asarray(P, float)
        N = self.N
        rows = self.rows(P)
        X, U = self.split_w(w)
        Xs = X[:-1].copy()
        Xs[0] = P[:NX]
        Z = np.concatenate([Xs, U], axis=1)
        Jac, gl = self.jac(Z, rows), self.grad_l(Z, rows)
        lam_g = np.asarray(lam_g, float).reshape(N + 1, NX)
        lam_x = np.asarray(lam_x, float)
        r = np.zeros(NX + NZ * N)
        ix = lambda k: np.arange(NX) if k == 0 else NX + NZ * (k - 1) + NU + np.arange(NX)  # noqa: E731
        r[ix(0)] -= lam_g[0]
        for k in range(N):
            l1 = lam_g[k + 1]
            if k > 0:
                r[ix(k)] += gl[k, :NX] + Jac[k, :, :NX].T @ l1
            r[NX + NZ * k: NX + NZ * k + NU] += gl[k, NX:] + Jac[k, :, NX:].T @ l1
            r[ix(k + 1)] -= l1
        r += lam_x
        g = np.concatenate([P[:NX] - X[0]] + [self.F(Z[k], rows[k]) - X[k + 1] for k in range(N)])
        lb, ub = self.bounds_w()
        w = np.asarray(w, float)
        viol = max(float(np.max(lb - w)), float(np.max(w - ub)), 0.0)
        up, dn = np.maximum(lam_x, 0.0), np.maximum(-lam_x, 0.0)
        sign = max(float(np.max(np.where(np.isfinite(ub), 0.0, up))), float(np.max(np.where(np.isfinite(lb), 0.0, dn))))
        du = np.where(np.isfinite(ub), ub - w, 0.0)
        dl = np.where(np.isfinite(lb), w - lb, 0.0)
        compl = max(float(np.max(up * np.abs(du))), float(np.max(dn * np.abs(dl))))
        return {"stat": float(np.max(np.abs(r))), "feas": float(np.max(np.abs(g))), "bound": viol, "sign": sign,
                "compl": compl}

    def objective(self, w, P):
        P = np.asarray(P, float)
        X, U = self.split_w(w)
        Xs = X[:-1].copy()
        Xs[0] = P[:NX]
        return float(np.sum(self.l(np.concatenate([Xs, U], axis=1), self.rows(P))))
