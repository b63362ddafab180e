"""NumPy references of the directional sensitivities of the MPC solution to the whole parameter row
(x0 and the references): the kernel csrc/sens.h sens_p_kernel.

A parameter direction is the KKT matrix of the sensitivities to x0 (helpers/sens_ref.py) with another
right-hand side.  Per direction (column): dx0 = dX_0, and per stage k < N
    r_k = d(grad_{z_k} l_k)/dp . dp   (nz),      d_k = d f_k/dp . dp   (nx),
so that the system is
    (H_k + Sigma_k) dz_k + [A_k B_k]^T lam_{k+1} - [lam_k; 0] + r_k = 0,
    A_k dX_k + B_k dU_k + d_k - dX_{k+1} = 0,      Sigma_x dX_N - lam_N = 0,      dX_0 = dx0.

(a) ``affine_sens``: the recursion, in float64 or np.longdouble -- backward from p_N = 0
        s = p_{k+1} + P_{k+1} d_k,  gx = r^x_k + A_k^T s,  gu = r^u_k + B_k^T s,
        kf_k = -Huu'_k^-1 gu,  p_k = gx + K_k^T gu,
    forward dU_k = K_k dX_k + kf_k, dX_{k+1} = A_k dX_k + B_k dU_k + d_k.
(b) ``dense_kkt_sens``: the same system assembled and solved densely (rows equilibrated).
(c) ``active_set_sens_p``: the parametric active-set reference -- active variables fixed, every other
    Sigma dropped, the dense KKT system with the right-hand side (-r, dx0).
(d) ``refined_sens_p``: one step of the kernel's iterative refinement restated with right-hand sides.

Layouts as in sens_ref.py; r (N, nz, m), d (N, nx, m), dx0 (nx, m); results (n_w, m) in the w layout.
"""
import numpy as np
import sens_ref as sr
from sens_ref import _solve, iu_w, ix_w


def _factors(A, B, H, Sig, dtype):
    """(P[0..N], K, Huu', Hd, regular) of the backward Riccati sweep of sens_ref.riccati_sens in ``dtype``."""
    N, nx = A.shape[0], A.shape[1]
    P = [None] * (N + 1)
    P[N] = np.diag(Sig[N, :nx])
    K, Huu, Hd = [None] * N, [None] * N, [None] * N
    regular = True
    for k in range(N - 1, -1, -1):
        Hd[k] = H[k] + np.diag(Sig[k] if k else np.concatenate([np.zeros(nx, dtype), Sig[k, nx:]]))
        PA, PB = P[k + 1] @ A[k], P[k + 1] @ B[k]
        Hux = Hd[k][nx:, :nx] + B[k].T @ PA
        Huu[k] = Hd[k][nx:, nx:] + B[k].T @ PB
        regular = regular and bool(np.all(np.linalg.eigvalsh(np.asarray(Huu[k], np.float64)) > 0))
        K[k] = -_solve(Huu[k], Hux)
        Pk = Hd[k][:nx, :nx] + A[k].T @ PA + Hux.T @ K[k]
        P[k] = (Pk + Pk.T) / 2
    return P, K, Huu, Hd, regular


def _pack(dX, dU, nx, nu, dtype):
    N, m = len(dU), dX[0].shape[1]
    dw = np.zeros((nx + (nx + nu) * N, m), dtype)
    for k in range(N + 1):
        dw[ix_w(nx, nu, k)] = dX[k]
    for k in range(N):
        dw[iu_w(nx, nu, k)] = dU[k]
    return dw


def _sweeps(A, B, P, K, Huu, rq, rr, d, x_start):
    """The Riccati solve of right-hand sides (rq[0..N], rr[0..N-1], d[0..N-1]) with given factors:
    (dX, dU, p) from dX_0 = x_start."""
    N = A.shape[0]
    p = [None] * (N + 1)
    p[N] = rq[N]
    kf = [None] * N
    for k in range(N - 1, -1, -1):
        s = p[k + 1] + P[k + 1] @ d[k]
        gu = rr[k] + B[k].T @ s
        kf[k] = -_solve(Huu[k], gu)
        p[k] = rq[k] + A[k].T @ s + K[k].T @ gu
    dX, dU = [x_start], []
    for k in range(N):
        dU.append(K[k] @ dX[k] + kf[k])
        dX.append(A[k] @ dX[k] + B[k] @ dU[k] + d[k])
    return dX, dU, p


def affine_sens(A, B, H, Sig, r, d, dx0, dtype=np.float64):
    """(dw (n_w, m), regular): recursion (a) in ``dtype``."""
    A, B, H, Sig, r, d, dx0 = (np.asarray(v, dtype) for v in (A, B, H, Sig, r, d, dx0))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P, K, Huu, _, regular = _factors(A, B, H, Sig, dtype)
    rq = [r[k][:nx] for k in range(N)] + [np.zeros_like(dx0)]
    rr = [r[k][nx:] for k in range(N)]
    dX, dU, _ = _sweeps(A, B, P, K, Huu, rq, rr, d, dx0)
    return _pack(dX, dU, nx, nu, dtype), regular


def refined_sens_p(A, B, H, Sig, r, d, dx0, resid_dtype=np.longdouble):
    """(dw before, dw after) one step of the kernel's refinement with right-hand sides, restated: the
    float64 recursion (a), the residuals of the full system at its result -- costates lam_k = P_k dX_k +
    p_k; r_k, d_k and dX_0 included -- summed in ``resid_dtype`` and rounded to float64, and the float64
    Riccati solve of them with the same factors from a zero dX_0."""
    A, B, H, Sig, r, d, dx0 = (np.asarray(v, np.float64) for v in (A, B, H, Sig, r, d, dx0))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P, K, Huu, Hd, _ = _factors(A, B, H, Sig, np.float64)
    rq = [r[k][:nx] for k in range(N)] + [np.zeros_like(dx0)]
    rr = [r[k][nx:] for k in range(N)]
    dX, dU, p = _sweeps(A, B, P, K, Huu, rq, rr, d, dx0)
    before = _pack(dX, dU, nx, nu, np.float64)
    R = lambda v: np.asarray(v, resid_dtype)  # noqa: E731
    lam = [P[k] @ dX[k] + p[k] for k in range(N + 1)]
    eq = [None] * N + [np.asarray(R(P[N]) @ R(dX[N]) - R(lam[N]), np.float64)]
    er, ed = [None] * N, [None] * N
    for k in range(N):
        eq[k] = np.asarray(R(Hd[k][:nx, :nx]) @ R(dX[k]) + R(Hd[k][:nx, nx:]) @ R(dU[k]) + R(A[k]).T @ R(lam[k + 1])
                           - R(lam[k]) + R(rq[k]), np.float64)
        er[k] = np.asarray(R(Hd[k][nx:, :nx]) @ R(dX[k]) + R(Hd[k][nx:, nx:]) @ R(dU[k]) + R(B[k]).T @ R(lam[k + 1])
                           + R(rr[k]), np.float64)
        ed[k] = np.asarray(R(A[k]) @ R(dX[k]) + R(B[k]) @ R(dU[k]) + R(d[k]) - R(dX[k + 1]), np.float64)
    cX, cU, _ = _sweeps(A, B, P, K, Huu, eq, er, ed, np.zeros_like(dx0))
    after = _pack([x + c for x, c in zip(dX, cX)], [u + c for u, c in zip(dU, cU)], nx, nu, np.float64)
    return before, after


def _kkt(A, B, Hd, r, d, dx0):
    """Dense KKT system of the stages Hd (Sigma included or not): (Hw, J, -r in the w layout, constraint rhs)."""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    nw, ng, m = nx + (nx + nu) * N, nx * (N + 1), dx0.shape[1]
    Hw, J = np.zeros((nw, nw)), np.zeros((ng, nw))
    gw, rhs = np.zeros((nw, m)), np.zeros((ng, m))
    J[:nx, :nx] = np.eye(nx)
    rhs[:nx] = dx0
    for k in range(N):
        iz = np.concatenate([ix_w(nx, nu, k), iu_w(nx, nu, k)])
        Hw[np.ix_(iz, iz)] += Hd[k]
        gw[iz] -= r[k]
        rows = nx * (k + 1) + np.arange(nx)
        J[np.ix_(rows, ix_w(nx, nu, k + 1))] = np.eye(nx)
        J[np.ix_(rows, ix_w(nx, nu, k))] = -A[k]
        J[np.ix_(rows, iu_w(nx, nu, k))] = -B[k]
        rhs[rows] = d[k]
    return Hw, J, gw, rhs


def _solve_free(Hw, J, gw, rhs, free):
    """(dw, condition number): the KKT system on the variables `free`, its rows scaled to unit max-norm
    (the solution is that of the unscaled system; a Sigma of 1e9 would otherwise set the conditioning)."""
    nf, ng = free.size, J.shape[0]
    Kkt = np.zeros((nf + ng, nf + ng))
    Kkt[:nf, :nf] = Hw[np.ix_(free, free)]
    Kkt[:nf, nf:] = J[:, free].T
    Kkt[nf:, :nf] = J[:, free]
    R = np.concatenate([gw[free], rhs])
    sc = 1.0 / np.max(np.abs(Kkt), axis=1)
    Kkt, R = Kkt * sc[:, None], R * sc[:, None]
    sol = np.linalg.solve(Kkt, R)
    dw = np.zeros((Hw.shape[0], R.shape[1]))
    dw[free] = sol[:nf]
    return dw, float(np.linalg.cond(Kkt))


def dense_kkt_sens(A, B, H, Sig, r, d, dx0):
    """(dw, cond): system (b), the barrier Sigma left in, float64."""
    A, B, H, Sig, r, d, dx0 = (np.asarray(v, np.float64) for v in (A, B, H, Sig, r, d, dx0))
    N, nx = A.shape[0], A.shape[1]
    Hd = [H[k] + np.diag(Sig[k] if k else np.concatenate([np.zeros(nx), Sig[k, nx:]])) for k in range(N)]
    Hw, J, gw, rhs = _kkt(A, B, Hd, r, d, dx0)
    xN = ix_w(nx, B.shape[2], N)
    Hw[xN, xN] += Sig[N, :nx]
    return _solve_free(Hw, J, gw, rhs, np.arange(Hw.shape[0]))


def active_set_sens_p(A, B, H, active, r, d, dx0):
    """dw (n_w, m) of the parametric active-set problem (c): min 1/2 dw^T H dw + r^T dw subject to
    dX_0 = dx0, dX_{k+1} = A_k dX_k + B_k dU_k + d_k and dw_i = 0 on the active variables (float64).
    active (n_w,) bool in the w layout (X_0's entries must be False)."""
    A, B, H, r, d, dx0 = (np.asarray(v, np.float64) for v in (A, B, H, r, d, dx0))
    active = np.asarray(active, bool)
    Hw, J, gw, rhs = _kkt(A, B, H, r, d, dx0)
    assert active.shape == (Hw.shape[0],) and not active[:A.shape[1]].any()
    return _solve_free(Hw, J, gw, rhs, np.flatnonzero(~active))[0]


def random_rhs(nx, nu, N, seed, m=None):
    """Seeded normal right-hand sides (r, d = 0, dx0) of m (default nx) directions."""
    rng = np.random.default_rng(seed + 2000)
    m = nx if m is None else m
    return rng.normal(size=(N, nx + nu, m)), np.zeros((N, nx, m)), rng.normal(size=(nx, m))


def linear_rhs(lin, dP, b=0):
    """(r, d, dx0) of a LinearOCP for the directions dP (m, n_p) of instance b's parameter row:
    r_k = -2 W_j dzr_k with dzr_k the direction's stage reference, d = 0, dx0 = dP[:, :nx]."""
    dP = np.atleast_2d(np.asarray(dP))
    nx, nz, N, m = lin.nx, lin.nx + lin.nu, lin.N, dP.shape[0]
    tab = lin.tab if lin.tab.ndim == 1 else lin.tab[b]
    dzr = dP[:, nx:].reshape(m, N, nz)
    dt = dP.dtype
    r = np.stack([-2 * np.asarray(lin.W[tab[k]], dt) @ dzr[:, k].T for k in range(N)])
    return r, np.zeros((N, nx, m), dt), dP[:, :nx].T.copy()


_E_REF_P = []


def e_ref_p():
    """The yardstick: the worst relative error of the float64 recursion (a) against the long-double one
    over LQ_SHAPES x LQ_SIGMAS (Sigma on a random 40 % of the inputs; seeded normal r and dx0, nx
    directions); computed once."""
    if not _E_REF_P:
        worst = 0.0
        for s, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
            A, B, H = sr.random_lq(nx, nu, N, s)
            r, d, dx0 = random_rhs(nx, nu, N, s)
            for sg in sr.LQ_SIGMAS:
                Sig = np.where(sr.random_input_mask(nx, nu, N, s), sg, 0.0)
                d64, ok = affine_sens(A, B, H, Sig, r, d, dx0, np.float64)
                dld, _ = affine_sens(A, B, H, Sig, r, d, dx0, np.longdouble)
                assert ok
                worst = max(worst, sr.rel_err(d64, dld))
        _E_REF_P.append(worst)
    return _E_REF_P[0]
