"""NumPy references of the sensitivities of the MPC solution to the initial state x0.

(a) ``riccati_sens``: the recursion of the sensitivity kernel (csrc/sens.h) restated from given stage
    operands (A_k, B_k, H_k, Sigma_k), in float64 or np.longdouble -- one backward Riccati sweep on
    H + Sigma from P_N = Sigma_x, the gains K_k (K_0 kept), then Phi_0 = I, Phi_{k+1} = (A_k + B_k K_k)
    Phi_k, dX_k = Phi_k, dU_k = K_k Phi_k.
(b) ``active_set_sens``: the active-set reference -- the variables classed active are fixed, every
    other Sigma is dropped, and the reduced KKT system is solved densely.  (A dense solve with the
    barrier Sigma left in is no reference: at Sigma >= 1e8 it is off by 1e-5 and worse.)

Layout: z_k = (x_k, u_k), H_k (nz, nz) over z_k, Sigma (N + 1, nz) with row k = (Sigma of X_k, Sigma
of U_k) (X_0 free: its entries are not read; row N holds X_N's only); results in the interleaved w
layout [X_0 | U_0 X_1 | ... | U_{N-1} X_N], row = index in w.
"""
import numpy as np

INF_BOUND = 1e19


def ix_w(nx, nu, k):
    """indices of X_k in w"""
    return np.arange(nx) if k == 0 else nx + (nx + nu) * (k - 1) + nu + np.arange(nx)


def iu_w(nx, nu, k):
    """indices of U_k in w"""
    return nx + (nx + nu) * k + np.arange(nu)


def _solve(M, R):
    """M^-1 R by Gaussian elimination with partial pivoting in the operands' dtype (np.linalg has no long double)."""
    M, R = M.copy(), R.copy()
    n = M.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]], R[[c, p]] = M[[p, c]], R[[p, c]]
        for r in range(c + 1, n):
            f = M[r, c] / M[c, c]
            M[r, c:] -= f * M[c, c:]
            R[r] -= f * R[c]
    X = np.zeros_like(R)
    for r in range(n - 1, -1, -1):
        X[r] = (R[r] - M[r, r + 1:] @ X[r + 1:]) / M[r, r]
    return X


def riccati_sens(A, B, H, Sig, dtype=np.float64):
    """(dw (n_w, nx), regular): the kernel's recursion in ``dtype``.  A (N, nx, nx), B (N, nx, nu),
    H (N, nz, nz), Sig (N + 1, nz).  regular = every reduced Huu' is positive definite."""
    A, B, H, Sig = (np.asarray(v, dtype) for v in (A, B, H, Sig))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P = np.diag(Sig[N, :nx])
    K = np.zeros((N, nu, nx), dtype)
    regular = True
    for k in range(N - 1, -1, -1):
        Hd = H[k] + np.diag(Sig[k])
        if k == 0:  # X_0 is free (and P_0 is not needed)
            Hd = H[k] + np.diag(np.concatenate([np.zeros(nx, dtype), Sig[k, nx:]]))
        PA, PB = P @ A[k], P @ B[k]
        Hxx = Hd[:nx, :nx] + A[k].T @ PA
        Hux = Hd[nx:, :nx] + B[k].T @ PA
        Huu = Hd[nx:, nx:] + B[k].T @ PB
        regular = regular and bool(np.all(np.linalg.eigvalsh(np.asarray(Huu, np.float64)) > 0))
        K[k] = -_solve(Huu, Hux)
        P = Hxx + Hux.T @ K[k]
        P = (P + P.T) / 2
    dw = np.zeros((nx + (nx + nu) * N, nx), dtype)
    Phi = np.eye(nx, dtype=dtype)
    dw[ix_w(nx, nu, 0)] = Phi
    for k in range(N):
        dw[iu_w(nx, nu, k)] = K[k] @ Phi
        Phi = (A[k] + B[k] @ K[k]) @ Phi
        dw[ix_w(nx, nu, k + 1)] = Phi
    return dw, regular


def refined_sens(A, B, H, Sig, resid_dtype=np.longdouble):
    """(dw before, dw after) one step of the kernel's iterative refinement, restated: the float64
    recursion, the KKT residuals of its result (costates lam_k = P_k dX_k) summed in ``resid_dtype``
    and rounded to float64, and the float64 Riccati solve of them with the same gains and P_k --
    backward p_N = rq_N, p_k = rq_k + A^T s + K^T (rr_k + B^T s) with s = p_{k+1} + P_{k+1} d_k,
    kf_k = -Huu'^-1 (rr_k + B^T s); forward ddX_0 = 0, ddU = K ddX + kf, ddX+ = A ddX + B ddU + d."""
    A, B, H, Sig = (np.asarray(v, np.float64) for v in (A, B, H, Sig))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P = [None] * (N + 1)
    P[N] = np.diag(Sig[N, :nx])
    K, Huu, Hd = [None] * N, [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Hd[k] = H[k] + np.diag(Sig[k] if k else np.concatenate([np.zeros(nx), Sig[k, nx:]]))
        PA, PB = P[k + 1] @ A[k], P[k + 1] @ B[k]
        Hux = Hd[k][nx:, :nx] + B[k].T @ PA
        Huu[k] = Hd[k][nx:, nx:] + B[k].T @ PB
        K[k] = -_solve(Huu[k], Hux)
        Pk = Hd[k][:nx, :nx] + A[k].T @ PA + Hux.T @ K[k]
        P[k] = (Pk + Pk.T) / 2
    dX, dU = [np.eye(nx)], []
    for k in range(N):
        dU.append(K[k] @ dX[k])
        dX.append((A[k] + B[k] @ K[k]) @ dX[k])

    def pack(dX, dU):
        dw = np.zeros((nx + (nx + nu) * N, nx))
        for k in range(N + 1):
            dw[ix_w(nx, nu, k)] = dX[k]
        for k in range(N):
            dw[iu_w(nx, nu, k)] = dU[k]
        return dw

    before = pack(dX, dU)
    R = lambda v: np.asarray(v, resid_dtype)  # noqa: E731
    lam = [P[k] @ dX[k] for k in range(N + 1)]
    rq = [None] * N + [np.asarray(R(P[N]) @ R(dX[N]) - R(lam[N]), np.float64)]
    rr, d = [None] * N, [None] * N
    for k in range(N):
        rq[k] = np.asarray(R(Hd[k][:nx, :nx]) @ R(dX[k]) + R(Hd[k][:nx, nx:]) @ R(dU[k])
                           + R(A[k]).T @ R(lam[k + 1]) - R(lam[k]), np.float64)
        rr[k] = np.asarray(R(Hd[k][nx:, :nx]) @ R(dX[k]) + R(Hd[k][nx:, nx:]) @ R(dU[k])
                           + R(B[k]).T @ R(lam[k + 1]), np.float64)
        d[k] = np.asarray(R(A[k]) @ R(dX[k]) + R(B[k]) @ R(dU[k]) - R(dX[k + 1]), np.float64)
    p, kf = rq[N], [None] * N
    for k in range(N - 1, -1, -1):
        s = p + P[k + 1] @ d[k]
        hu = rr[k] + B[k].T @ s
        kf[k] = -_solve(Huu[k], hu)
        p = rq[k] + A[k].T @ s + K[k].T @ hu
    ddx = np.zeros((nx, nx))
    for k in range(N):
        ddu = K[k] @ ddx + kf[k]
        dU[k] = dU[k] + ddu
        ddx = A[k] @ ddx + B[k] @ ddu + d[k]
        dX[k + 1] = dX[k + 1] + ddx
    return before, pack(dX, dU)


def active_set_sens(A, B, H, active):
    """dw (n_w, nx) of the active-set problem: min 1/2 dw^T H dw subject to dX_0 = dx0, dX_{k+1} =
    A_k dX_k + B_k dU_k and dw_i = 0 on the active variables; the reduced KKT system solved densely
    (float64).  active (n_w,) bool in the w layout (X_0's entries must be False)."""
    A, B, H = (np.asarray(v, np.float64) for v in (A, B, H))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    nw, ng = nx + (nx + nu) * N, nx * (N + 1)
    active = np.asarray(active, bool)
    assert active.shape == (nw,) and not active[:nx].any()
    Hw, J, rhs = np.zeros((nw, nw)), np.zeros((ng, nw)), np.zeros((ng, nx))
    J[:nx, :nx] = np.eye(nx)
    rhs[:nx] = np.eye(nx)
    for k in range(N):
        iz = np.concatenate([ix_w(nx, nu, k), iu_w(nx, nu, k)])
        Hw[np.ix_(iz, iz)] += H[k]
        r = nx * (k + 1) + np.arange(nx)
        J[np.ix_(r, ix_w(nx, nu, k + 1))] = np.eye(nx)
        J[np.ix_(r, ix_w(nx, nu, k))] = -A[k]
        J[np.ix_(r, iu_w(nx, nu, k))] = -B[k]
    free = np.flatnonzero(~active)
    nf = free.size
    Kkt = np.zeros((nf + ng, nf + ng))
    Kkt[:nf, :nf] = Hw[np.ix_(free, free)]
    Kkt[:nf, nf:] = J[:, free].T
    Kkt[nf:, :nf] = J[:, free]
    sol = np.linalg.solve(Kkt, np.concatenate([np.zeros((nf, nx)), rhs]))
    dw = np.zeros((nw, nx))
    dw[free] = sol[:nf]
    return dw


def classify(w, lam_x, lbw, ubw, nx):
    """(active, ok) of one instance's bounded variables: active = slack < 1e-6 and |lam_x| > 1e-2
    (class i); ok = every bounded variable is in class (i) or has |lam_x| < 1e-7 (class ii)."""
    w, lam_x, lbw, ubw = (np.asarray(v, np.float64) for v in (w, lam_x, lbw, ubw))
    bounded = (lbw > -INF_BOUND) | (ubw < INF_BOUND)
    bounded[:nx] = False
    slack = np.minimum(np.where(lbw > -INF_BOUND, w - lbw, np.inf), np.where(ubw < INF_BOUND, ubw - w, np.inf))
    active = bounded & (slack < 1e-6) & (np.abs(lam_x) > 1e-2)
    inactive = bounded & (np.abs(lam_x) < 1e-7)
    return active, bool(np.all(~bounded | active | inactive))


def sigma_of(w, lam_x, lbw, ubw, nx, nu, dtype=np.float64):
    """Sigma (N + 1, nz) of one instance from its point and bounds, as the kernel forms it:
    zL / (w - lb) + zU / (ub - w) with zU = max(lam_x, 0), zL = max(-lam_x, 0); 0 without a finite
    bound and on X_0."""
    w, lam_x, lbw, ubw = (np.asarray(v, dtype) for v in (w, lam_x, lbw, ubw))
    N = (w.size - nx) // (nx + nu)
    zero = np.zeros_like(w)
    one = np.ones_like(w)
    hl, hu = lbw > -INF_BOUND, ubw < INF_BOUND
    s = np.where(hl, np.maximum(-lam_x, zero) / np.where(hl, w - lbw, one), zero)
    s = s + np.where(hu, np.maximum(lam_x, zero) / np.where(hu, ubw - w, one), zero)
    Sig = np.zeros((N + 1, nx + nu), dtype)
    for k in range(N + 1):
        if k > 0:
            Sig[k, :nx] = s[ix_w(nx, nu, k)]
        if k < N:
            Sig[k, nx:] = s[iu_w(nx, nu, k)]
    return Sig


def linear_operands(lin, b=0):
    """(A, B, H) per stage of a LinearOCP for instance b: its tables along the schedule, H = 2 W."""
    tab = lin.tab if lin.tab.ndim == 1 else lin.tab[b]
    return lin.A[tab], lin.B[tab], 2.0 * lin.W[tab]


def ocp_bounds(lin):
    """(lbw, ubw) of a problem (its u_lb / u_ub / x_lb / x_ub) in the w layout, +-1e20 = no bound."""
    nx, nu, N = lin.nx, lin.nu, lin.N
    fin = lambda v, inf: np.array([x if np.isfinite(x) else inf for x in v], float)  # noqa: E731
    lb, ub = np.full(nx + (nx + nu) * N, -1e20), np.full(nx + (nx + nu) * N, 1e20)
    for k in range(N):
        lb[iu_w(nx, nu, k)], ub[iu_w(nx, nu, k)] = fin(lin.u_lb, -1e20), fin(lin.u_ub, 1e20)
        lb[ix_w(nx, nu, k + 1)], ub[ix_w(nx, nu, k + 1)] = fin(lin.x_lb, -1e20), fin(lin.x_ub, 1e20)
    return lb, ub


LQ_SHAPES = ((3, 2, 5), (3, 2, 20), (4, 1, 50), (5, 1, 50), (4, 2, 12))  # (nx, nu, N)
LQ_SIGMAS = (1.0, 1e4, 1e9)


def random_lq(nx, nu, N, seed):
    """Random LQ stages: A_k of spectral radius 0.95, B_k normal, H_k symmetric positive definite
    (eigenvalues >= 0.5) over z = (x, u)."""
    rng = np.random.default_rng(seed)
    nz = nx + nu
    A = rng.normal(size=(N, nx, nx))
    A *= (0.95 / np.max(np.abs(np.linalg.eigvals(A)), axis=1))[:, None, None]
    B = rng.normal(size=(N, nx, nu))
    M = rng.normal(size=(N, nz, nz)) / np.sqrt(nz)
    H = M @ np.swapaxes(M, 1, 2) + 0.5 * np.eye(nz)
    return A, B, H


def random_input_mask(nx, nu, N, seed, frac=0.4):
    """(N + 1, nz) bool: a random `frac` of the inputs (none of the states)"""
    rng = np.random.default_rng(seed + 1000)
    m = np.zeros((N + 1, nx + nu), bool)
    m[:N, nx:] = rng.random((N, nu)) < frac
    return m


_E_REF = []


def e_ref():
    """The yardstick E_ref: the worst relative error of the float64 recursion against the long-double
    one over LQ_SHAPES x LQ_SIGMAS (Sigma on a random 40 % of the inputs); computed once."""
    if not _E_REF:
        worst = 0.0
        for s, (nx, nu, N) in enumerate(LQ_SHAPES):
            A, B, H = random_lq(nx, nu, N, s)
            for sg in LQ_SIGMAS:
                Sig = np.where(random_input_mask(nx, nu, N, s), sg, 0.0)
                d64, ok = riccati_sens(A, B, H, Sig, np.float64)
                dld, _ = riccati_sens(A, B, H, Sig, np.longdouble)
                assert ok
                worst = max(worst, rel_err(d64, dld))
        _E_REF.append(worst)
    return _E_REF[0]


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|) over the entries"""
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
