"""CPU tests of the long-double references of the sensitivity calls on the nonlinear models
(tests/helpers/sens_nonlinear_ref.py), which tests/test_gpu_sens_nonlinear.py holds the kernels of csrc/sens.h to.
Nothing here runs the kernels: the points are the CPU oracle's solutions (oracle.ipm_ref.solve) of the cases of
tests/test_gpu_sens.py (nonlinear_problem) and the tracking unicycle of tests/test_gpu_sens_p.py.  The
path-frame bicycle, which the oracle does not solve, gets a seeded feasible point (a roll-out of seeded inputs
inside the bounds by helpers/path_bicycle_ref.py, which yields no multipliers) with seeded multipliers.

1. the hyper-dual unicycle (both costs) against the C++ oracle's analytic stage derivatives;
2. stationarity of the assembled operands: the sign and index conventions of the multipliers and of stage 0;
3. independent routes: the long-double recursion against a dense KKT solve, the reverse references against the
   forward ones through the dot-product identities;
4. the reference has teeth: a Gauss-Newton Hessian or a stage 0 evaluated 1e-6 off moves it by far more than
   the bound of the GPU test;
5. the yardsticks E64(case, call), printed and asserted <= 1e-12.
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import sens_nonlinear_ref as sn  # noqa: E402
import sens_p_ref as sp  # noqa: E402
import sens_ref as sr  # noqa: E402
import stage_derivs_ref as sd  # noqa: E402
from test_gpu_sens import NONLINEAR_CASES  # noqa: E402
from test_gpu_sens_p import nonlinear_p_problem  # noqa: E402

LD = np.longdouble
EPS = 2.0 ** -52
CASES = NONLINEAR_CASES + ("unicycle_tracking_N10",)


def calls_of(ocp):
    """sens_p and sens_vjp refuse the path-frame bicycle"""
    return tuple(c for c in sn.CALLS if not (sn.model_of(ocp) == "path_bicycle" and c in ("p", "vjp")))


def directions(call, ocp, n_p, seed, m=None):
    """The arguments of a call after the bounds: m (default nx) seeded normal directions or cotangents over the
    whole row, shaped as the Solver's for one instance."""
    nx, nu, N = ocp.nx, ocp.nu, ocp.N
    nw = nx + (nx + nu) * N
    m = nx if m is None else m
    rng = np.random.default_rng(seed + 7 * sn.CALLS.index(call))
    if call == "x0":
        return ()
    if call == "p":
        return (rng.normal(size=(m, n_p)),)
    if call == "bounds":
        return rng.normal(size=(m, nw)), rng.normal(size=(m, nw))
    if call == "weights":  # relative to each weight (where it is not zero): a unit direction of the cart-pole's
        # R = 1e-4 moves the solution by 1e5, and the entries of O(1) next to those lose E64 <= 1e-12 (3.8e-12)
        Q, R = (np.where(np.array(v, float) > 0, np.array(v, float), 1.0) for v in (ocp.Q, ocp.R))
        return rng.normal(size=(m, N, nx)) * Q[:nx], rng.normal(size=(m, N, nu)) * R[:nu]
    return (rng.normal(size=(m, nw)),)


def path_point(ocp, P):
    """A seeded feasible point of the path-frame bicycle with seeded multipliers: inputs inside half their box,
    the states their roll-out (every defect zero, the steering inside its box: asserted), lam_g normal at the
    size of the cost's gradient, lam_x zero (no variable is near a bound)."""
    import path_bicycle_ref as pb

    pr = pb.PathProblem(ocp)
    rng = np.random.default_rng(77)
    B = P.shape[0]
    w, lam_g = np.zeros((B, ocp.n_w_ms)), np.zeros((B, ocp.n_g_ms))
    for b in range(B):
        U = rng.uniform(-0.5, 0.5, (ocp.N, 2)) * np.array([0.1 * ocp.u_ub[0], ocp.u_ub[1]])
        X = pr.rollout(U, P[b, :4], pr.rows(P[b]))
        assert np.all(np.abs(X[:, 3]) < 0.9 * ocp.x_ub[3])
        w[b] = pr.join_w(X, U)
        lam_g[b, 4:] = 0.1 * rng.normal(size=4 * ocp.N)
    return {"w": w, "lam_g": lam_g, "lam_x": np.zeros_like(w), "status": np.zeros(B, np.int32)}


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    """(ocp, P, point, lb, ub, tol): the oracle's solution of a case (shared; never modified)"""
    from oracle import ipm_ref

    ocp, P, opts = nonlinear_p_problem(name)
    lb, ub = sr.ocp_bounds(ocp)
    if sn.model_of(ocp) == "path_bicycle":
        r = path_point(ocp, P)
    else:
        r = ipm_ref.solve(ocp, P, lbw=lb, ubw=ub, **opts)
        assert np.all(r["status"] <= 1), (name, r["status"])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ocp, P, r, lb, ub, opts.get("tol", 1e-8)


def sol_of(r, b):
    return {k: r[k][b] for k in ("w", "lam_g", "lam_x")}


@functools.lru_cache(maxsize=None)
def points_of(name):
    """the long-double and float64 sens_nonlinear_ref.Point of every instance of a case"""
    ocp, P, r, lb, ub, _ = cpu_case(name)
    return list(zip(sn.points(ocp, P, r, lb, ub, LD), sn.points(ocp, P, r, lb, ub, np.float64)))


@functools.lru_cache(maxsize=None)
def yardsticks(name):
    """{call: (E64, references per instance)} of a case: the worst instance's float64-against-long-double distance"""
    ocp, P, r, lb, ub, _ = cpu_case(name)
    out = {}
    for call in calls_of(ocp):
        worst, refs = 0.0, []
        for b, (pt, pt64) in enumerate(points_of(name)):
            e, ref, ok = sn.e64(call, ocp, P[b], sol_of(r, b), lb, ub, directions(call, ocp, P.shape[1], 100 + b), pt, pt64)
            assert ok, (name, call, b, "the reference's own factors are not regular")
            worst = max(worst, e)
            refs.append(ref)
        out[call] = (worst, refs)
    return out


# ------------------------------------------------------------------------------------------
# 1. the hyper-dual unicycle against the C++ oracle's analytic derivatives
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unicycle_points(n=256):
    rng = np.random.default_rng(1001)
    U = lambda lo, hi: rng.uniform(lo, hi, n)  # noqa: E731
    Z = np.stack([U(-2, 2), U(-2, 2), U(-np.pi, np.pi), U(-1.5, 1.5), U(-1.2, 1.2)], axis=1)
    zr = Z + rng.normal(0, 0.3, Z.shape)
    lam = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    return Z, lam, zr


@pytest.mark.parametrize("with_lam", [True, False], ids=["lam", "lam0"])
@pytest.mark.parametrize("cost,M", [("quadrature", 4), ("node", 1), ("node", 4)])
def test_unicycle_derivatives_against_the_oracle(cost, M, with_lam):
    """The unicycle of helpers/stage_derivs_ref.py (restated from oracle/nlp_ref.py) against ipm_ref.stage -- the
    C++ oracle's analytic xf, q, Jacobian and Hessian of q + lam^T xf -- at 256 seeded points, block by block as
    stage_derivs_ref.block_errors measures, within tests/test_gpu_stage_derivs.py's bound max(16 E64, 4 * 2^-52).
    Measured (E64 / oracle's error, with lam): quadrature M = 4 xf 3.9e-16/3.9e-16 q 1.3e-15/1.3e-15 A
    8.4e-17/8.4e-17 B 4.3e-16/4.3e-16 g 6.0e-15/6.0e-15 H 6.0e-16/7.1e-16; node M = 4 the same but q 2.8e-16, g
    1.1e-16, H 5.0e-16 on both sides; node M = 1 smaller throughout.  (The oracle's float64 formulas round as the
    float64 hyper-dual pass does in every block but the quadrature's H.)"""
    from oracle import ipm_ref, nlp_ref

    Z, lam, zr = unicycle_points()
    if not with_lam:
        lam = np.zeros_like(lam)
    Q, R, T = (1.0, 5.0, 0.1), (0.5, 0.05), 0.2
    ref = sd.stage_derivs("unicycle", Z, lam, zr, 1.0, T, M, Q, R, (), LD, cost=cost)
    f64 = sd.stage_derivs("unicycle", Z, lam, zr, 1.0, T, M, Q, R, (), np.float64, cost=cost)
    xf, qf, jac, hess = ipm_ref.stage(nlp_ref.UnicycleOCP(N=1, T=T, M=M, Q=Q, R=R, cost=cost), Z[:, :3], Z[:, 3:],
                                      zr[:, :3], zr[:, 3:], lam)
    got = {"xf": xf, "q": qf, "A": jac[:, :3, :3], "B": jac[:, :3, 3:], "g": jac[:, 3, :], "H": hess}
    E, err = sd.block_errors(f64, ref), sd.block_errors(got, ref)
    print(f"\nunicycle {cost} M={M} lam={with_lam}: " + " ".join(f"{b} E64 {E[b]:.1e} oracle {err[b]:.1e}" for b in sd.BLOCKS))
    for b in sd.BLOCKS:
        assert err[b] <= max(16 * E[b], 4 * EPS), (b, err[b], E[b])


# ------------------------------------------------------------------------------------------
# 2. stationarity of the assembled operands
# ------------------------------------------------------------------------------------------
def stationarity(ocp, P_b, sol, sign=1.0):
    """max over the rows of |grad q_k + [A_k B_k]^T lam_{k+1} - lam_k + lam_x|: the X rows of stages 1..N-1 and of
    node N (-lam_N + lam_x), the U rows of every stage -- stage 0's U rows alone, X_0 being pinned by g_0."""
    nx, nu, N = sn.dims(ocp)
    Z, zr = sn.stage_points(ocp, P_b, sol["w"], LD)
    lam = sign * sn.multipliers(ocp, sol["lam_g"], LD)
    d = sd.stage_derivs(sn.model_of(ocp), Z, lam, zr, 1.0, ocp.T, ocp.M, ocp.Q, ocp.R, getattr(ocp, "par", ()), LD,
                        cost=ocp.cost)
    lx = np.asarray(sol["lam_x"], LD)
    worst = float(np.max(np.abs(-lam[N - 1] + lx[sr.ix_w(nx, nu, N)])))
    for k in range(N):
        gu = d["g"][k, nx:] + d["B"][k].T @ lam[k] + lx[sr.iu_w(nx, nu, k)]
        worst = max(worst, float(np.max(np.abs(gu))))
        if k > 0:
            gx = d["g"][k, :nx] + d["A"][k].T @ lam[k] - lam[k - 1] + lx[sr.ix_w(nx, nu, k)]
            worst = max(worst, float(np.max(np.abs(gx))))
    return worst


@pytest.mark.parametrize("name", [c for c in CASES if c != "path_bicycle_N20"])
def test_stationarity_of_the_assembled_operands(name):
    """At the oracle's solutions the operands' own first-order conditions hold within 100 x the solve's tol on every
    row -- with stage k's multiplier lam_g[nx (k + 1) : nx (k + 2)] taken with a plus sign and stage 0 evaluated at
    (P[:nx], U_0); with the other sign they are off by 1e-2 and more (asserted: the check can tell).  (The
    path-frame bicycle's point is no solution; its conventions are the other ODE models'.)  Measured: 1.2e-15 to
    2.6e-9 (kin_bicycle_N10 the largest), the other sign 0.23 to 5.5."""
    ocp, P, r, _, _, tol = cpu_case(name)
    for b in range(P.shape[0]):
        good, bad = stationarity(ocp, P[b], sol_of(r, b)), stationarity(ocp, P[b], sol_of(r, b), -1.0)
        print(f"{name} b={b}: stationarity {good:.3e} (tol {tol:.0e}), with the other sign {bad:.3e}")
        assert good <= 100.0 * tol
        assert bad > 1e-2


# ------------------------------------------------------------------------------------------
# 3. independent routes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_recursion_against_the_dense_kkt_solve(name):
    """sens_ref.riccati_sens in long double on the assembled operands equals sens_p_ref.dense_kkt_sens (float64,
    rows equilibrated) of the same system with dx0 = I, at the instances without an active bound (Sigma <= 1).
    Bound: the dense solve's own, n cond(KKT) 2^-52 for its n unknowns (Gaussian elimination with partial
    pivoting, no growth assumed), relative to max(1, |entry|).  Measured: 1.5e-15 (path-frame bicycle) to 2.9e-13
    (cart-pole) against bounds of 3.3e-12 to 7.4e-11; every instance of the unicycle cases has active bounds and
    is passed over."""
    ocp, P, r, lb, ub, _ = cpu_case(name)
    nx, nu, N = sn.dims(ocp)
    seen = 0
    for b, (pt, _) in enumerate(points_of(name)):
        if float(np.max(pt.Sig)) > 1.0:
            continue
        seen += 1
        rec, ok = sr.riccati_sens(pt.A, pt.B, pt.H, pt.Sig, LD)
        assert ok
        zr_, zd = np.zeros((N, nx + nu, nx)), np.zeros((N, nx, nx))
        dense, cond = sp.dense_kkt_sens(pt.A, pt.B, pt.H, pt.Sig, zr_, zd, np.eye(nx))
        err, n = sr.rel_err(dense, rec), rec.shape[0] + nx * (N + 1)
        print(f"{name} b={b}: recursion against the dense solve {err:.3e} (cond {cond:.2e}, bound {n * cond * EPS:.2e})")
        assert err <= n * cond * EPS
    assert seen > 0 or name.startswith("unicycle"), "the ODE cases have no active bound"


def identity_terms(args, fwd, rev_args, rev):
    """(<g, dw>, <gradient, direction>, scale) (m_g, m_d) each in long double; scale = sum |g| max(1, |dw|) +
    sum max(1, |gradient|) |direction|, the form of the GPU tests' identity_gap"""
    g = np.asarray(rev_args[0], LD)
    big = lambda v: np.maximum(1.0, np.abs(v))  # noqa: E731
    lhs, sc = g @ fwd, np.abs(g) @ big(fwd)
    # sens_p: (gP, dP); bounds: (glbw, dlbw), (gubw, dubw); weights: (gQk, dQ), (gRk, dR)
    pairs = list(zip(rev, args))
    rhs = np.zeros_like(lhs)
    for grad, d in pairs:
        grad, d = np.asarray(grad, LD).reshape(g.shape[0], -1), np.asarray(d, LD).reshape(fwd.shape[1], -1)
        rhs, sc = rhs + grad @ d.T, sc + big(grad) @ np.abs(d).T
    return lhs, rhs, sc


@pytest.mark.parametrize("name", CASES)
def test_reverse_references_against_the_forward_ones(name):
    """<g, dw> = <gradient, direction> in long double for the three pairs (sens_p / sens_vjp, the bounds pair, the
    weights pair), nx seeded directions against nx seeded cotangents over the whole rows.  Bound: both sides carry
    the long-double pipeline's own rounding, 2^-11 of the float64 pipeline's E64 (the formats' mantissas: 64
    against 53 bits), so 64 x 2^-11 x max(E64 of the two calls, their linear yardsticks) x the scale of
    identity_terms.  (Directions of the bounds where there is none count for nothing on either side.)
    Measured: the worst gap / bound per case and pair 1.2e-5 to 8.6e-4 where bounds are active or the pair is not
    the bounds' (without an active bound both sides of the bounds' identity are the barrier's O(mu): 5e-11 and
    below)."""
    ocp, P, r, lb, ub, _ = cpu_case(name)
    Y = yardsticks(name)
    hl, hu = lb > -sr.INF_BOUND, ub < sr.INF_BOUND
    hl[:ocp.nx] = hu[:ocp.nx] = False
    for fwd_call, rev_call in (("p", "vjp"), ("bounds", "bounds_vjp"), ("weights", "weights_vjp")):
        if fwd_call not in calls_of(ocp):
            continue
        unit = 64.0 * 2.0 ** -11 * max(Y[fwd_call][0], Y[rev_call][0], sn.linear_yardstick(fwd_call),
                                       sn.linear_yardstick(rev_call))
        worst = 0.0
        for b, (pt, _) in enumerate(points_of(name)):
            args = directions(fwd_call, ocp, P.shape[1], 100 + b)
            if fwd_call == "bounds":
                args = (np.where(hl, args[0], 0.0), np.where(hu, args[1], 0.0))
            rev_args = directions(rev_call, ocp, P.shape[1], 100 + b)
            fwd = sn._REFERENCE[fwd_call](ocp, P[b], sol_of(r, b), lb, ub, *args, dtype=LD, at=pt)[0]
            rev = sn._REFERENCE[rev_call](ocp, P[b], sol_of(r, b), lb, ub, *rev_args, dtype=LD, at=pt)
            lhs, rhs, sc = identity_terms(args, fwd, rev_args, rev)
            worst = max(worst, float(np.max(np.abs(lhs - rhs) / (unit * sc))))
        print(f"{name} {fwd_call} / {rev_call}: worst identity gap / bound {worst:.3e} (unit {unit:.2e})")
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------
# 4. the reference has teeth
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_reference_has_teeth(name):
    """Two deliberately wrong variants of the operands move dw*/dx0 by more than 1000 x the GPU test's bound of the
    case, 64 max(E64(case, x0), e_ref): (a) H at lam = 0 (a Gauss-Newton Hessian: every curvature term of the
    dynamics missing), (b) stage 0 evaluated at x0 + 1e-6 (the wrong node's state by that little).  The worst
    instance of the case counts, as for the GPU test's error.  Measured (a, b): unicycle_N10 1.1, 3.6e-6;
    unicycle_bounded_N10 1.4, 6.0e-6; unicycle_N30 2.2, 2.7e-6; kin_bicycle_N10 1.1, 2.8e-6; cartpole_N20 0.31,
    2.9e-6; path_bicycle_N20 1.3e-2, 2.8e-7; dyn_bicycle_N10 0.82, 2.0e-6; unicycle_tracking_N10 1.0, 2.3e-6 --
    against 1000 x bound = 3.9e-11 to 1.8e-10."""
    ocp, P, r, lb, ub, _ = cpu_case(name)
    E, refs = yardsticks(name)["x0"]
    need = 1000.0 * 64.0 * max(E, sr.e_ref())
    moved = {"gauss_newton": 0.0, "stage0": 0.0}
    for b in range(P.shape[0]):
        n = refs[b].size
        for key, variant in (("gauss_newton", {"gauss_newton": True}), ("stage0", {"stage0": r["w"][b, :ocp.nx] + 1e-6})):
            pt = sn.Point(ocp, P[b], sol_of(r, b), lb, ub, LD, **variant)
            if not pt.regular:  # (a Gauss-Newton Hessian may even lose definiteness: moved beyond any bound)
                moved[key] = np.inf
                continue
            dw = sn.reference_x0(ocp, P[b], sol_of(r, b), lb, ub, LD, at=pt)[0]
            moved[key] = max(moved[key], sr.rel_err(np.ravel(dw), refs[b][:n]))
    print(f"{name}: Gauss-Newton H moves dw/dx0 by {moved['gauss_newton']:.3e}, stage 0 at x0 + 1e-6 by "
          f"{moved['stage0']:.3e}; 1000 x the GPU bound = {need:.3e}")
    assert moved["gauss_newton"] > need and moved["stage0"] > need


# ------------------------------------------------------------------------------------------
# 5. the yardsticks
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_yardsticks(name):
    """E64(case, call): the float64 pipeline (float64 hyper-dual operands, the float64 recursion with its
    refinement round) against the long-double one, relative to max(1, |entry|), worst instance.  A reference
    that is itself ill-conditioned is no reference: E64 <= 1e-12.  Measured: 4.6e-17 to 3.6e-15 on seven of the
    cases, the cart-pole 2.9e-15 (x0) to 7.9e-14 (p); the bounds pair of the ODE cases, whose picks have no
    active bound, 1e-22 and below (an O(mu) result against max(1, |entry|)).  node-cost G_k is -2 W (asserted: the mixed
    hyper-dual pass finds what include/mpcx.h states)."""
    ocp, P, r, lb, ub, _ = cpu_case(name)
    Y = yardsticks(name)
    print(f"{name}: E64 " + "  ".join(f"{c} {Y[c][0]:.2e}" for c in Y))
    for c in Y:
        assert Y[c][0] <= 1e-12, (name, c)
    if ocp.cost == "node" and sn.model_of(ocp) != "path_bicycle":
        nx, nz = ocp.nx, ocp.nx + ocp.nu
        W = np.diag(np.array(list(ocp.Q)[:nx] + list(ocp.R)[:ocp.nu], LD))
        if ocp.param == "x0_xref":
            W[:, nx:] = 0
        G = points_of(name)[0][0].G
        assert sr.rel_err(G, np.broadcast_to(-2 * W, G.shape)) <= 2.0 ** -60 and G.shape[1:] == (nz, nz)
