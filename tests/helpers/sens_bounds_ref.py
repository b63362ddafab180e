"""NumPy references of the sensitivities of the MPC solution to the box bounds (the kernels csrc/sens.h
sens_bnd_kernel and sens_bnd_vjp_kernel).

The system is that of helpers/sens_p_ref.py,
    (H_k + Sigma_k) dz_k + [A_k B_k]^T lam_{k+1} - [lam_k; 0] + r_k = 0,   Sigma_x dX_N - lam_N + rq_N = 0,
    A_k dX_k + B_k dU_k - dX_{k+1} = 0,   dX_0 = 0,
and with the products zL_i (w_i - lb_i), zU_i (ub_i - w_i) held fixed a direction (dlb, dub) of the bounds,
each shaped like w, gives
    r_i = -(sigL_i dlb_i + sigU_i dub_i),   sigL_i = zL_i / (w_i - lb_i),   sigU_i = zU_i / (ub_i - w_i)
on every bounded variable, the X rows of node N included; Sigma = sigL + sigU.  The reverse mode: with
z~ the adjoint solve of helpers/sens_vjp_ref.py for a cotangent g,  g_lb = -sigL z~,  g_ub = -sigU z~.

(a) ``bounds_sens``: the recursion (sens_p_ref._factors / _sweeps with rq_N), float64 or np.longdouble.
(b) ``dense_kkt_bounds``: the same system assembled and solved densely.
(c) ``refined_solve`` / ``refined_bounds_sens`` / ``refined_bounds_vjp``: one step of the kernel's iterative
    refinement, restated; ``reference``: both rounds in long double.
(d) ``active_set_bounds``: active variables move with their bound (dw_i = dbound_i), every other Sigma
    dropped, the rest solved densely.
(e) ``bounds_vjp``: the reverse formulas.
(f) ``barrier_lq``: a fixed-mu barrier LQ problem solved by Newton's method, for central differences.

Layouts as in sens_ref.py; sigL, sigU (n_w,) and dlb, dub, g (n_w, m) in the w layout (X_0's entries of
sigL / sigU are zero); results (n_w, m).
"""
import numpy as np
import sens_p_ref as sp
import sens_ref as sr
from sens_ref import INF_BOUND, iu_w, ix_w


def split_sigma(w, lam_x, lbw, ubw, nx, dtype=np.float64):
    """(sigL, sigU) (n_w,) of one instance as the kernels form them: zL = max(-lam_x, 0), zU = max(lam_x, 0),
    0 without a finite bound and on X_0."""
    w, lam_x, lbw, ubw = (np.asarray(v, dtype) for v in (w, lam_x, lbw, ubw))
    zero, one = np.zeros_like(w), np.ones_like(w)
    hl, hu = lbw > -INF_BOUND, ubw < INF_BOUND
    sL = np.where(hl, np.maximum(-lam_x, zero) / np.where(hl, w - lbw, one), zero)
    sU = np.where(hu, np.maximum(lam_x, zero) / np.where(hu, ubw - w, one), zero)
    sL[:nx] = 0
    sU[:nx] = 0
    return sL, sU


def stage_sigma(s, nx, nu):
    """Sigma (N + 1, nz) of sens_ref's layout from a (n_w,) vector in the w layout."""
    N = (s.size - nx) // (nx + nu)
    Sig = np.zeros((N + 1, nx + nu), s.dtype)
    for k in range(N + 1):
        if k > 0:
            Sig[k, :nx] = s[ix_w(nx, nu, k)]
        if k < N:
            Sig[k, nx:] = s[iu_w(nx, nu, k)]
    return Sig


def bound_rhs(sigL, sigU, dlb, dub, nx, nu):
    """(rq[0..N], rr[0..N-1], d[0..N-1]) of the directions: r = -(sigL dlb + sigU dub), rq_0 = 0, d = 0."""
    r = -(sigL[:, None] * dlb + sigU[:, None] * dub)
    r[:nx] = 0
    N = (sigL.size - nx) // (nx + nu)
    rq = [r[ix_w(nx, nu, k)] for k in range(N + 1)]
    rr = [r[iu_w(nx, nu, k)] for k in range(N)]
    return rq, rr, [np.zeros_like(rq[0]) for _ in range(N)]


def _operands(A, B, H, sigL, sigU, dtype):
    A, B, H, sigL, sigU = (np.asarray(v, dtype) for v in (A, B, H, sigL, sigU))
    return A, B, H, sigL, sigU, stage_sigma(sigL + sigU, A.shape[1], B.shape[2])


def bounds_sens(A, B, H, sigL, sigU, dlb, dub, dtype=np.float64):
    """(dw (n_w, m), regular): recursion (a) in ``dtype``."""
    A, B, H, sigL, sigU, Sig = _operands(A, B, H, sigL, sigU, dtype)
    dlb, dub = np.asarray(dlb, dtype), np.asarray(dub, dtype)
    nx, nu = A.shape[1], B.shape[2]
    P, K, Huu, _, regular = sp._factors(A, B, H, Sig, dtype)
    rq, rr, d = bound_rhs(sigL, sigU, dlb, dub, nx, nu)
    dX, dU, _ = sp._sweeps(A, B, P, K, Huu, rq, rr, d, np.zeros_like(rq[0]))
    return sp._pack(dX, dU, nx, nu, dtype), regular


def refined_solve(A, B, H, Sig, rq, rr, dtype=np.float64, resid_dtype=np.longdouble):
    """((X, U) before, (X, U) after, regular) one step of the kernel's refinement on the Riccati solve of the
    right-hand sides (rq[0..N], rr[0..N-1], d = 0) from a zero start, restated as
    sens_p_ref.refined_sens_p with the right-hand side of node N in its residual: the solve in ``dtype``,
    the residuals summed in ``resid_dtype`` and rounded to ``dtype``.  With both np.longdouble this is the
    kernels' two rounds restated in long double -- the reference of the GPU tests: a Sigma of 1e9 on a
    STATE makes Huu' = R + B^T P B ill-conditioned where the KKT system is not, and the plain recursion
    then loses up to 1e9 roundings of its own precision, long double included (6e-11); the round takes
    them out."""
    N, nx = A.shape[0], A.shape[1]
    P, K, Huu, Hd, regular = sp._factors(A, B, H, Sig, dtype)
    zero = np.zeros_like(rq[0])
    d = [zero for _ in range(N)]
    dX, dU, p = sp._sweeps(A, B, P, K, Huu, rq, rr, d, zero)
    R = lambda v: np.asarray(v, resid_dtype)  # noqa: E731
    lam = [P[k] @ dX[k] + p[k] for k in range(N + 1)]
    eq = [None] * N + [np.asarray(R(P[N]) @ R(dX[N]) - R(lam[N]) + R(rq[N]), dtype)]
    er, ed = [None] * N, [None] * N
    for k in range(N):
        eq[k] = np.asarray(R(Hd[k][:nx, :nx]) @ R(dX[k]) + R(Hd[k][:nx, nx:]) @ R(dU[k]) + R(A[k]).T @ R(lam[k + 1])
                           - R(lam[k]) + R(rq[k]), dtype)
        er[k] = np.asarray(R(Hd[k][nx:, :nx]) @ R(dX[k]) + R(Hd[k][nx:, nx:]) @ R(dU[k]) + R(B[k]).T @ R(lam[k + 1])
                           + R(rr[k]), dtype)
        ed[k] = np.asarray(R(A[k]) @ R(dX[k]) + R(B[k]) @ R(dU[k]) - R(dX[k + 1]), dtype)
    cX, cU, _ = sp._sweeps(A, B, P, K, Huu, eq, er, ed, zero)
    return (dX, dU), ([x + c for x, c in zip(dX, cX)], [u + c for u, c in zip(dU, cU)]), regular


def refined_bounds_sens(A, B, H, sigL, sigU, dlb, dub, resid_dtype=np.longdouble, dtype=np.float64):
    """(dw before, dw after) the refinement round (``refined_solve``) on the bound right-hand sides."""
    A, B, H, sigL, sigU, Sig = _operands(A, B, H, sigL, sigU, dtype)
    nx, nu = A.shape[1], B.shape[2]
    rq, rr, _ = bound_rhs(sigL, sigU, np.asarray(dlb, dtype), np.asarray(dub, dtype), nx, nu)
    b, a, _ = refined_solve(A, B, H, Sig, rq, rr, dtype, resid_dtype)
    return sp._pack(*b, nx, nu, dtype), sp._pack(*a, nx, nu, dtype)


def refined_bounds_vjp(A, B, H, sigL, sigU, g, resid_dtype=np.longdouble, dtype=np.float64):
    """(g_lb, g_ub) of reference (e) after the refinement round on the adjoint solve."""
    import sens_vjp_ref as sv

    A, B, H, sigL, sigU, Sig = _operands(A, B, H, sigL, sigU, dtype)
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    rq, rr, _ = sv._rhs_of(np.asarray(g, dtype), nx, nu, N)
    _, a, _ = refined_solve(A, B, H, Sig, rq, rr, dtype, resid_dtype)
    zt = sp._pack(*a, nx, nu, dtype)
    return -sigL[:, None] * zt, -sigU[:, None] * zt


def reference(A, B, H, sigL, sigU, dlb, dub):
    """dw of the kernel's two rounds restated in long double (residuals in long double too)."""
    return refined_bounds_sens(A, B, H, sigL, sigU, dlb, dub, np.longdouble, np.longdouble)[1]


def dense_kkt_bounds(A, B, H, sigL, sigU, dlb, dub):
    """(dw, cond): system (b), the barrier Sigma left in, float64."""
    A, B, H, sigL, sigU, Sig = _operands(A, B, H, sigL, sigU, np.float64)
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    m = np.asarray(dlb).shape[1]
    Hd = [H[k] + np.diag(Sig[k] if k else np.concatenate([np.zeros(nx), Sig[k, nx:]])) for k in range(N)]
    Hw, J, _, rhs = sp._kkt(A, B, Hd, np.zeros((N, nx + nu, m)), np.zeros((N, nx, m)), np.zeros((nx, m)))
    xN = ix_w(nx, nu, N)
    Hw[xN, xN] += Sig[N, :nx]
    gw = sigL[:, None] * np.asarray(dlb, np.float64) + sigU[:, None] * np.asarray(dub, np.float64)  # -r
    gw[:nx] = 0
    return sp._solve_free(Hw, J, gw, rhs, np.arange(Hw.shape[0]))


def active_set_bounds(A, B, H, active, dbound):
    """dw (n_w, m) of reference (d): dw_i = dbound_i on the active variables (dbound (n_w, m): the direction
    of the bound each is active on), min 1/2 dw^T H dw subject to the dynamics and dX_0 = 0 over the rest."""
    A, B, H, dbound = (np.asarray(v, np.float64) for v in (A, B, H, dbound))
    active = np.asarray(active, bool)
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    m = dbound.shape[1]
    Hw, J, _, _ = sp._kkt(A, B, H, np.zeros((N, nx + nu, m)), np.zeros((N, nx, m)), np.zeros((nx, m)))
    assert active.shape == (Hw.shape[0],) and not active[:nx].any()
    fixed = np.where(active[:, None], dbound, 0.0)
    dw, _ = sp._solve_free(Hw, J, -(Hw @ fixed), -(J @ fixed), np.flatnonzero(~active))
    return dw + fixed


def adjoint_z(A, B, H, Sig, g, dtype):
    """z~ (n_w, m) in the w layout and `regular`: the adjoint solve of sens_vjp_ref (rq = gX on every node,
    rr = gU, zero start)."""
    import sens_vjp_ref as sv

    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    P, K, Huu, _, regular = sp._factors(A, B, H, Sig, dtype)
    rq, rr, d = sv._rhs_of(g, nx, nu, N)
    X, U, _ = sp._sweeps(A, B, P, K, Huu, rq, rr, d, np.zeros_like(rq[0]))
    return sp._pack(X, U, nx, nu, dtype), regular


def bounds_vjp(A, B, H, sigL, sigU, g, dtype=np.float64):
    """(g_lb (n_w, m), g_ub (n_w, m), regular): reference (e) in ``dtype``."""
    A, B, H, sigL, sigU, Sig = _operands(A, B, H, sigL, sigU, dtype)
    zt, regular = adjoint_z(A, B, H, Sig, np.asarray(g, dtype), dtype)
    return -sigL[:, None] * zt, -sigU[:, None] * zt, regular


# ---------------------------------------------------------------------------------------------------
# seeded problems
# ---------------------------------------------------------------------------------------------------
def random_bound_mask(nx, nu, N, seed, states=True):
    """(lower (n_w,), upper (n_w,)) bool: which variables carry a lower / an upper bound -- at most one side
    each: sens_ref.random_input_mask's 40 % of the inputs and, with ``states``, state 0 of node N and state
    1 % nx of node N // 2 + 1 (one state per node at most: with more bounded states than inputs to steer
    them the KKT system itself degenerates as Sigma grows); the side by a seeded coin."""
    rng = np.random.default_rng(seed + 3000)
    nw = nx + (nx + nu) * N
    um = sr.random_input_mask(nx, nu, N, seed)
    has = np.zeros(nw, bool)
    for k in range(N):
        has[iu_w(nx, nu, k)] = um[k, nx:]
    if states:
        has[ix_w(nx, nu, N)[0]] = True
        has[ix_w(nx, nu, N // 2 + 1)[1 % nx]] = True
    side = rng.random(nw) < 0.5
    return has & side, has & ~side


def random_directions(nx, nu, N, seed, m=None):
    """Seeded normal (dlb, dub) (n_w, m) each, m default nx."""
    rng = np.random.default_rng(seed + 5000)
    nw = nx + (nx + nu) * N
    m = nx if m is None else m
    return rng.normal(size=(nw, m)), rng.normal(size=(nw, m))


_E_REF_B = []


def _e_ref_pair():
    if not _E_REF_B:
        import sens_vjp_ref as sv

        fwd = rev = 0.0
        for s, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
            A, B, H = sr.random_lq(nx, nu, N, s)
            lo, up = random_bound_mask(nx, nu, N, s, states=False)
            dlb, dub = random_directions(nx, nu, N, s)
            g = sv.random_cotangent(nx, nu, N, s)
            for sg in sr.LQ_SIGMAS:
                sL, sU = np.where(lo, sg, 0.0), np.where(up, sg, 0.0)
                d64, ok = bounds_sens(A, B, H, sL, sU, dlb, dub, np.float64)
                dld, _ = bounds_sens(A, B, H, sL, sU, dlb, dub, np.longdouble)
                assert ok
                fwd = max(fwd, sr.rel_err(d64, dld))
                v64, vld = bounds_vjp(A, B, H, sL, sU, g, np.float64), bounds_vjp(A, B, H, sL, sU, g, np.longdouble)
                assert v64[2]
                # (relative to the multiplier's scale: g_lb = -sigL z~ with sigL up to 1e9 and z~ ~ 1 / sigL)
                rev = max(rev, sr.rel_err(np.concatenate(v64[:2]), np.concatenate(vld[:2])))
        _E_REF_B.extend([fwd, rev])
    return _E_REF_B


def e_ref_b():
    """The yardstick of the forward mode, computed as sens_p_ref.e_ref_p is: the worst relative error
    (sens_ref.rel_err) of the float64 recursion (a) against the long-double one over LQ_SHAPES x LQ_SIGMAS
    (Sigma on a random 40 % of the inputs, as there) with the bound right-hand sides (the side of each bound
    by a seeded coin; nx seeded normal directions of either bound); computed once."""
    return _e_ref_pair()[0]


def e_ref_bvjp():
    """The yardstick of the reverse mode: the same for reference (e) with nx seeded normal cotangents."""
    return _e_ref_pair()[1]


# ---------------------------------------------------------------------------------------------------
# (f) a fixed-mu barrier LQ problem
# ---------------------------------------------------------------------------------------------------
def barrier_lq(A, B, H, c, x0, lb, ub, mu, w_start, tol=1e-12, max_iter=200):
    """Newton's method on  min 1/2 w^T Hw w + c^T w - mu sum log(w - lb) - mu sum log(ub - w)  subject to the
    dynamics and X_0 = x0 (bounds beyond +-1e19: none; X_0 unbounded), from w_start strictly inside the
    bounds (the dynamics need not hold there).  Returns (w, lam_x = zU - zL with zL = mu / (w - lb),
    zU = mu / (ub - w), residual norm)."""
    A, B, H = (np.asarray(v, np.float64) for v in (A, B, H))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    Hw, J, _, rhs = sp._kkt(A, B, H, np.zeros((N, nx + nu, 1)), np.zeros((N, nx, 1)), np.asarray(x0, float)[:, None])
    rhs = rhs[:, 0]
    nw, ng = Hw.shape[0], J.shape[0]
    hl, hu = lb > -INF_BOUND, ub < INF_BOUND
    hl[:nx] = hu[:nx] = False
    w, lam = np.array(w_start, float), np.zeros(ng)

    def resid(w, lam):
        zL = np.where(hl, mu / np.where(hl, w - lb, 1.0), 0.0)
        zU = np.where(hu, mu / np.where(hu, ub - w, 1.0), 0.0)
        return np.concatenate([Hw @ w + c - zL + zU + J.T @ lam, J @ w - rhs]), zL, zU

    for _ in range(max_iter):
        F, zL, zU = resid(w, lam)
        nrm = float(np.max(np.abs(F)))
        if nrm <= tol:
            break
        Sg = np.where(hl, zL / np.where(hl, w - lb, 1.0), 0.0) + np.where(hu, zU / np.where(hu, ub - w, 1.0), 0.0)
        Kk = np.block([[Hw + np.diag(Sg), J.T], [J, np.zeros((ng, ng))]])
        step = np.linalg.solve(Kk, -F)
        dw, dl = step[:nw], step[nw:]
        a = 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            tl = np.where(hl & (dw < 0), -(w - lb) / dw, np.inf)
            tu = np.where(hu & (dw > 0), (ub - w) / dw, np.inf)
        a = min(1.0, 0.99 * float(min(tl.min(), tu.min())))
        while a > 1e-12 and float(np.max(np.abs(resid(w + a * dw, lam + a * dl)[0]))) > (1 - 1e-4 * a) * nrm:
            a *= 0.5
        w, lam = w + a * dw, lam + a * dl
    F, zL, zU = resid(w, lam)
    return w, zU - zL, float(np.max(np.abs(F)))
