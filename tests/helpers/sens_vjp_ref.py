"""NumPy references of the adjoint sensitivities of the MPC solution (the kernel csrc/sens.h
sens_vjp_kernel): gP = (dw*/dP)^T g for cotangents g shaped like w.

The forward system of helpers/sens_p_ref.py has the right-hand side (r_k, d_k, dx0) and the result
dw = (dX, dU).  Its KKT matrix is symmetric, so the transpose solve is the same Riccati solve of
right-hand sides with the same factors (sens_p_ref._factors / _sweeps) and the cotangent in their place:
    rq_k = gX_k  (k = 0..N, node N included),   rr_k = gU_k,   d = 0,   X~_0 = 0,
no sign flipped.  With its result (X~, U~, p~) and the costates lam~_k = P_k X~_k + p~_k,
    <g, dw> = lam~_0^T dx0 + sum_{k<N} ( z~_k^T r_k + lam~_{k+1}^T d_k ),     z~_k = (X~_k, U~_k),
for every (r, d, dx0): (lam~_0, z~_k, lam~_{k+1}) is the transpose of the Jacobian of dw with respect to
(dx0, r_k, d_k) applied to g.

(a) ``adjoint_sens``: the restatement, float64 or np.longdouble.
(b) ``contract``: <g, dw> from (a)'s result and a right-hand side, the identity above.
(c) ``linear_vjp``: the gradient row of a LinearOCP, gzr_k = -2 W_j z~_k.
(d) ``refined_adjoint``: one step of the kernel's iterative refinement, restated.
Layouts as in sens_ref.py; g (n_w, m).
"""
import numpy as np
import sens_p_ref as sp
import sens_ref as sr
from sens_ref import iu_w, ix_w


def _rhs_of(g, nx, nu, N):
    rq = [g[ix_w(nx, nu, k)] for k in range(N + 1)]
    rr = [g[iu_w(nx, nu, k)] for k in range(N)]
    d = [np.zeros_like(rq[0]) for _ in range(N)]
    return rq, rr, d


def adjoint_sens(A, B, H, Sig, g, dtype=np.float64):
    """(lam0 (nx, m), zt (N, nz, m), lamn (N, nx, m) = lam~_{k+1}, regular): restatement (a) in ``dtype``."""
    A, B, H, Sig, g = (np.asarray(v, dtype) for v in (A, B, H, Sig, g))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P, K, Huu, _, regular = sp._factors(A, B, H, Sig, dtype)
    rq, rr, d = _rhs_of(g, nx, nu, N)
    X, U, p = sp._sweeps(A, B, P, K, Huu, rq, rr, d, np.zeros_like(rq[0]))
    lam = [P[k] @ X[k] + p[k] for k in range(N + 1)]
    zt = np.stack([np.concatenate([X[k], U[k]]) for k in range(N)])
    return lam[0], zt, np.stack(lam[1:]), regular


def contract(lam0, zt, lamn, r, d, dx0):
    """(m_g, m) matrix of <g_i, dw_j> by the identity: lam~_0^T dx0 + sum_k (z~_k^T r_k + lam~_{k+1}^T d_k)."""
    out = lam0.T @ dx0
    for k in range(zt.shape[0]):
        out = out + zt[k].T @ r[k] + lamn[k].T @ d[k]
    return out


def linear_vjp(lin, lam0, zt, b=0):
    """gP (m, n_p) of a LinearOCP for instance b: gP[:nx] = lam~_0, gzr_k = G_k^T z~_k with G_k = -2 W_j
    (sens_p_ref.linear_rhs: r_k = -2 W_j dzr_k, d = 0)."""
    nx, nz, N, m = lin.nx, lin.nx + lin.nu, lin.N, lam0.shape[1]
    tab = lin.tab if lin.tab.ndim == 1 else lin.tab[b]
    dt = lam0.dtype
    gP = np.zeros((m, nx + nz * N), dt)
    gP[:, :nx] = lam0.T
    for k in range(N):
        gP[:, nx + nz * k:nx + nz * (k + 1)] = (-2 * np.asarray(lin.W[tab[k]], dt).T @ zt[k]).T
    return gP


def refined_adjoint(A, B, H, Sig, g, resid_dtype=np.longdouble):
    """((lam0, zt, lamn) before, (lam0, zt, lamn) after) one step of the kernel's refinement, restated as
    sens_p_ref.refined_sens_p: the float64 solve (a), the residuals of the full system at its result
    summed in ``resid_dtype`` and rounded to float64, the float64 Riccati solve of them with the same
    factors from a zero X~_0; the costates' offsets p~ take the correction's."""
    A, B, H, Sig, g = (np.asarray(v, np.float64) for v in (A, B, H, Sig, g))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P, K, Huu, Hd, _ = sp._factors(A, B, H, Sig, np.float64)
    rq, rr, d = _rhs_of(g, nx, nu, N)
    zero = np.zeros_like(rq[0])
    X, U, p = sp._sweeps(A, B, P, K, Huu, rq, rr, d, zero)

    def pack(X, U, p):
        lam = [P[k] @ X[k] + p[k] for k in range(N + 1)]
        return lam[0], np.stack([np.concatenate([X[k], U[k]]) for k in range(N)]), np.stack(lam[1:])

    before = pack(X, U, p)
    R = lambda v: np.asarray(v, resid_dtype)  # noqa: E731
    lam = [P[k] @ X[k] + p[k] for k in range(N + 1)]
    eq = [None] * N + [np.asarray(R(P[N]) @ R(X[N]) - R(lam[N]) + R(rq[N]), np.float64)]
    er, ed = [None] * N, [None] * N
    for k in range(N):
        eq[k] = np.asarray(R(Hd[k][:nx, :nx]) @ R(X[k]) + R(Hd[k][:nx, nx:]) @ R(U[k]) + R(A[k]).T @ R(lam[k + 1])
                           - R(lam[k]) + R(rq[k]), np.float64)
        er[k] = np.asarray(R(Hd[k][nx:, :nx]) @ R(X[k]) + R(Hd[k][nx:, nx:]) @ R(U[k]) + R(B[k]).T @ R(lam[k + 1])
                           + R(rr[k]), np.float64)
        ed[k] = np.asarray(R(A[k]) @ R(X[k]) + R(B[k]) @ R(U[k]) - R(X[k + 1]), np.float64)
    cX, cU, cp = sp._sweeps(A, B, P, K, Huu, eq, er, ed, zero)
    after = pack([x + c for x, c in zip(X, cX)], [u + c for u, c in zip(U, cU)], [a + c for a, c in zip(p, cp)])
    return before, after


def stack(lam0, zt, lamn):
    """one (nx + N nz + N nx, m) array of a result, for entrywise comparisons"""
    return np.concatenate([lam0, zt.reshape(-1, zt.shape[2]), lamn.reshape(-1, lamn.shape[2])])


def random_cotangent(nx, nu, N, seed, m=None):
    """Seeded normal cotangents over the whole of w, m (default nx) columns."""
    return np.random.default_rng(seed + 4000).normal(size=(nx + (nx + nu) * N, nx if m is None else m))


_E_REF_VJP = []


def e_ref_vjp():
    """The yardstick: the worst relative error (sens_ref.rel_err: relative to max(1, |entry|)) of the
    float64 restatement (a) against the long-double one over LQ_SHAPES x LQ_SIGMAS (Sigma on a random
    40 % of the inputs; nx seeded normal cotangents); computed once, as sens_p_ref.e_ref_p."""
    if not _E_REF_VJP:
        worst = 0.0
        for s, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
            A, B, H = sr.random_lq(nx, nu, N, s)
            g = random_cotangent(nx, nu, N, s)
            for sg in sr.LQ_SIGMAS:
                Sig = np.where(sr.random_input_mask(nx, nu, N, s), sg, 0.0)
                r64 = adjoint_sens(A, B, H, Sig, g, np.float64)
                rld = adjoint_sens(A, B, H, Sig, g, np.longdouble)
                assert r64[3]
                worst = max(worst, sr.rel_err(stack(*r64[:3]), stack(*rld[:3])))
        _E_REF_VJP.append(worst)
    return _E_REF_VJP[0]
