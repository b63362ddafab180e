"""GPU tests of the sensitivities of the MPC solution to the box bounds (mpcx_sens_bounds[_vjp][_dev],
Solver.sens_bounds / sens_bounds_vjp, DeviceLoop.sens_bounds / sens_bounds_vjp, mpcx.autograd with bounds;
csrc/sens.h sens_bnd_kernel, sens_bnd_vjp_kernel).

References: tests/helpers/sens_bounds_ref.py -- the kernel's two rounds restated in long double from the
GPU's own point, the active-set reference -- central differences of the solver itself under moved bounds
for the nonlinear models, and the project's forward mode for the reverse one, through the dot-product
identity <g, dw> = <g_lb, dlb> + <g_ub, dub>.  Cases are those of tests/test_gpu_sens.py (its constructors
and cached solves are imported) plus random bounded LQ problems at N = 15, 31, 63 with a state bound at
node N, which then sits on the last lane of its group."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sens_bounds_ref as sb  # noqa: E402
import sens_ref as sr  # noqa: E402
from test_gpu_sens import (LINEAR_CASES, NONLINEAR_CASES, REF_OPTS, linear_case, linear_problem,  # noqa: E402
                           nonlinear_problem, unicycle_P)

LD = np.longdouble


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def point_of(r, rows=slice(None)):
    return {k: r[k][rows] for k in ("w", "lam_g", "lam_x")}


def restated(A, Bm, H, w, lam_x, lb, ub, nx, dlb, dub):
    """the kernel's two rounds in long double at the GPU's own point: dlb, dub (m, n_w) -> dw (n_w, m)"""
    sL, sU = sb.split_sigma(w, lam_x, lb, ub, nx, LD)
    return sb.reference(A, Bm, H, sL, sU, np.asarray(dlb.T, LD), np.asarray(dub.T, LD))


def identity_gap(g, dw, gl, gu, dlb, dub):
    """(|<g, dw> - <g_lb, dlb> - <g_ub, dub>|, bound) per (instance, cotangent, direction), the 64 x e_ref form of
    tests/test_gpu_sens_vjp.py: g, gl, gu (B, mg, n_w), dw (B, n_w, md), dlb, dub (B, md, n_w); entries of the
    directions where the gradient is an exact zero (no finite bound there) do not count."""
    dl, du = np.where(gl[:, :1] == 0.0, 0.0, dlb), np.where(gu[:, :1] == 0.0, 0.0, dub)
    lhs = np.einsum("bci,bij->bcj", g, dw)
    rhs = np.einsum("bci,bji->bcj", gl, dl) + np.einsum("bci,bji->bcj", gu, du)
    big = lambda v: np.maximum(1.0, np.abs(v))  # noqa: E731
    bound = (64.0 * sb.e_ref_b() * np.einsum("bci,bij->bcj", np.abs(g), big(dw))
             + 64.0 * sb.e_ref_bvjp() * (np.einsum("bci,bji->bcj", big(gl), np.abs(dl))
                                         + np.einsum("bci,bji->bcj", big(gu), np.abs(du))))
    return np.abs(lhs - rhs), bound


# ------------------------------------------------------------------------------------------
# 1. linear cases: test_gpu_sens.py's solves, shared, never modified
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_bounds_case(name):
    """(lin, P, solve result, solver, dlb, dub (B, nx, n_w) seeded normal on every entry, sens_bounds result,
    g (B, nx, n_w) seeded normal, sens_bounds_vjp result)"""
    lin, P, r, _, solver = linear_case(name)
    rng = np.random.default_rng(500 + LINEAR_CASES.index(name))
    dlb, dub, g = (rng.normal(size=(P.shape[0], lin.nx, lin.n_w_ms)) for _ in range(3))
    s = solver.sens_bounds(P, r, dlb, dub)
    v = solver.sens_bounds_vjp(P, r, g)
    for a in (dlb, dub, g, *s.values(), *v.values()):
        a.setflags(write=False)
    return lin, P, r, solver, dlb, dub, s, g, v


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_restatement(mpcx, name):
    """1. The forward kernel against its two rounds restated in long double at the same point and tables, nx
    seeded normal directions on all bounded entries of either bound: 64 x e_ref_b relative to
    max(1, |entry|) (e_ref_b = 3.7e-15, so 2.4e-13).  Measured on one MI355X: padded_dint_N8 2.1e-16,
    lin4x2_N12 4.1e-16, ltv_N40 9.7e-17, cartpole_qp_N50 2.9e-26 (no bound active: |dw| <= 5e-10)."""
    lin, P, r, _, dlb, dub, s, _, _ = linear_bounds_case(name)
    tol = 64.0 * sb.e_ref_b()
    B = P.shape[0]
    assert np.all(s["flag"] == 0), s["flag"]
    assert s["dw"].shape == (B, lin.n_w_ms, lin.nx)
    lb, ub = sr.ocp_bounds(lin)
    worst = 0.0
    for b in range(B):
        A, Bm, H = sr.linear_operands(lin, b)
        ref = restated(A, Bm, H, r["w"][b], r["lam_x"][b], lb, ub, lin.nx, dlb[b], dub[b])
        worst = max(worst, sr.rel_err(s["dw"][b], ref))
        assert not s["dw"][b, :lin.nx].any()  # dX_0 = 0, exactly
    print(f"{name}: |dw| {np.abs(s['dw']).max():.3g}, worst error against the long-double restatement {worst:.3e} "
          f"(tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_active_set(mpcx, name):
    """1. Against the active-set reference (active variables move with their bound, every other Sigma dropped).
    Asserted on the inputs: strict complementarity by sens_ref.classify, and at least one active bound per
    case except the cart-pole QP.  Tolerance 8 x the restatement's own distance to the reference, as
    tests/test_gpu_sens.py::test_linear_against_the_active_set.  Measured on one MI355X: distances 2.7e-8 to
    8.7e-6, the GPU's equal to the restatement's to three digits in every instance."""
    lin, P, r, _, dlb, dub, s, _, _ = linear_bounds_case(name)
    lb, ub = sr.ocp_bounds(lin)
    n_act = 0
    for b in range(P.shape[0]):
        act, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, lin.nx)
        assert ok, (name, b, "a bounded variable is neither active nor without a multiplier")
        n_act += int(act.sum())
        A, Bm, H = sr.linear_operands(lin, b)
        dbound = np.where((r["lam_x"][b] < 0)[:, None], dlb[b].T, dub[b].T)  # the side it is active on
        ref = sb.active_set_bounds(A, Bm, H, act, dbound)
        rest = np.asarray(restated(A, Bm, H, r["w"][b], r["lam_x"][b], lb, ub, lin.nx, dlb[b], dub[b]), np.float64)
        dist = float(np.max(np.abs(rest - ref)))
        err = float(np.max(np.abs(s["dw"][b] - ref)))
        print(f"{name} b={b}: {int(act.sum())} active, restatement - active set {dist:.3e}, GPU - active set {err:.3e}")
        assert err <= 8.0 * dist
        if act.any():  # an active variable moves with its bound
            assert np.max(np.abs(s["dw"][b][act] - dbound[act])) <= 8.0 * dist
    assert n_act > 0 or name == "cartpole_qp_N50", "the case must have active bounds"


# ------------------------------------------------------------------------------------------
# 2. edge shapes: node N on the last lane of its group, several groups per wave, surplus lanes
# ------------------------------------------------------------------------------------------
def edge_state(lin):
    """index in w of the state of node N that the last input moves most (the bounded one)"""
    return sr.ix_w(lin.nx, lin.nu, lin.N)[int(np.argmax(np.abs(lin.B[0][:, 0])))]


@functools.lru_cache(maxsize=None)
def edge_case(N):
    """A random stable LQ problem (LinearModel<4,1>), B = 5, |u| <= 0.5, and per-instance bounds that put a
    one-sided bound on one state of node N (edge_state): 0.2 inside the free solution for instances 0..2 (active: lower
    for 0 and 2, upper for 1), 1 away from it for 3 and 4.  Returns (lin, P, lb, ub, result, solver)."""
    import mpcx
    from mpcx import lti

    rng = np.random.default_rng(700 + N)
    nx, nu, B = 4, 1, 5
    A = rng.normal(size=(nx, nx))
    A *= 0.95 / np.max(np.abs(np.linalg.eigvals(A)))
    Bm = rng.normal(size=(nx, nu))
    lin = lti.LinearOCP(N=N, A=A[None], B=Bm[None], W=np.diag([1.0, 2.0, 1.0, 0.5, 0.5])[None],
                        tab=np.zeros(N, np.int32), u_lb=(-0.5,), u_ub=(0.5,))
    P = lin.params(2.0 * rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    solver = mpcx.nlpsol(f"edge_N{N}", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    free = solver.solve_batch(P)
    assert np.all(free["status"] == 0), free["status"]
    lb0, ub0 = sr.ocp_bounds(lin)
    lb, ub = np.tile(lb0, (B, 1)), np.tile(ub0, (B, 1))
    j = edge_state(lin)
    xn = free["w"][:, j]
    lb[[0, 2], j] = xn[[0, 2]] + 0.2
    ub[1, j] = xn[1] - 0.2
    lb[3, j], ub[4, j] = xn[3] - 1.0, xn[4] + 1.0
    r = solver.solve_batch(P, lbw=lb, ubw=ub)
    assert np.all(r["status"] == 0), r["status"]
    for a in (lb, ub, *r.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return lin, P, lb, ub, r, solver


@pytest.mark.parametrize("N", [15, 31, 63])
def test_edge_shapes_against_the_restatement(mpcx, N):
    """2. N = 15, 31, 63: node N on lane G - 1 (where rq_N and from_next can go wrong), B = 5 (4, 2, 1 groups
    per wave: surplus lanes in the last wave), per-instance (B, n_w) bounds with a state bound at node N,
    active in three instances.  Forward against the long-double restatement, 64 x e_ref_b; the reverse mode
    through the identity against the forward one.  Measured on one MI355X, N = 15 / 31 / 63: 1.1e-16,
    2.0e-16, 4.7e-16 (tolerance 2.4e-13); identity gap / bound 2.0e-4, 5.4e-4, 5.3e-4."""
    lin, P, lb, ub, r, solver = edge_case(N)
    nx, nu, B = lin.nx, lin.nu, P.shape[0]
    rng = np.random.default_rng(800 + N)
    dlb, dub, g = (rng.normal(size=(B, nx, lin.n_w_ms)) for _ in range(3))
    s = solver.sens_bounds(P, r, dlb, dub, lbw=lb, ubw=ub)
    v = solver.sens_bounds_vjp(P, r, g, lbw=lb, ubw=ub)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    A, Bm, H = sr.linear_operands(lin)
    j = edge_state(lin)
    tol, worst = 64.0 * sb.e_ref_b(), 0.0
    for b in range(B):
        act, _ = sr.classify(r["w"][b], r["lam_x"][b], lb[b], ub[b], nx)
        assert bool(act[j]) == (b < 3), (b, act[j])
        ref = restated(A, Bm, H, r["w"][b], r["lam_x"][b], lb[b], ub[b], nx, dlb[b], dub[b])
        worst = max(worst, sr.rel_err(s["dw"][b], ref))
        if b < 3:  # node N's state moves with its bound (to the barrier term's O(mu))
            assert np.max(np.abs(s["dw"][b, j] - (dub[b, :, j] if b == 1 else dlb[b, :, j]))) < 1e-5
    gap, bound = identity_gap(g, s["dw"], v["glbw"], v["gubw"], dlb, dub)
    print(f"N={N}: worst error against the long-double restatement {worst:.3e} (tolerance {tol:.3e}); identity gap "
          f"{gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert worst <= tol
    assert np.all(gap <= bound)
    assert np.max(np.abs(v["glbw"][0, :, j])) > 1e-3 and not v["gubw"][0, :, j].any()


# ------------------------------------------------------------------------------------------
# 3. nonlinear models against central differences of the solver itself under moved bounds
# ------------------------------------------------------------------------------------------
def seeded_directions(name, lb, ub, B, nx):
    """(dlb, dub) (B, 2, n_w): column 0 seeded normal on the bounded entries, column 1 the uniform tightening
    dlb = +1, dub = -1 on the input bounds; zero where there is no finite bound and on X_0."""
    rng = np.random.default_rng(600 + NONLINEAR_CASES.index(name))
    n_w = lb.size
    hl, hu = lb > -sr.INF_BOUND, ub < sr.INF_BOUND
    hl[:nx] = hu[:nx] = False
    dlb, dub = rng.normal(size=(B, 2, n_w)), rng.normal(size=(B, 2, n_w))
    dlb[:, 1], dub[:, 1] = 1.0, -1.0
    return np.where(hl, dlb, 0.0), np.where(hu, dub, 0.0)


@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_nonlinear_against_finite_differences(mpcx, name):
    """3. dw against central differences of solve_batch(P, lbw = lb +- h dlb, ubw = ub +- h dub) along two
    seeded directions (one the uniform tightening of the input bounds), warm-started from the nominal
    solution, at h = 1e-3 and 1e-4.  Yardstick and tolerance as tests/test_gpu_sens.py: 4 x the spread of
    the two estimates + 1e-6 against their mean; an instance whose active set changes under +- h is left
    out, at most one per case; the nominal solutions are strictly complementary (asserted).  All seven
    models, the path-frame and the 6-state bicycle included.

    The solver of this test runs at tol = 1e-10 (the cases' other options kept).  At the cases' own 1e-8 a
    warm-started solve under a moved bound stops one iteration early, the same way at either h, so the two
    estimates agree with each other (spread 2.6e-6 on instance 3 of unicycle_N30) and are both off: there
    the estimate of dU_7 was -0.466994779 at every h from 1e-3 to 1e-6, the kernel's value -0.467014724
    (2.0e-5 apart, against a tolerance of 1.1e-5), and at tol = 1e-10 and 1e-12 the estimate is -0.467016221
    and the kernel's value -0.467016222.  The spread is a yardstick only of errors that depend on h.
    Measured on one MI355X at tol = 1e-10, worst instance of each case (spread, |GPU - FD|): unicycle_N10
    5.7e-6, 2.9e-6; unicycle_bounded_N10 6.3e-5, 3.2e-5; unicycle_N30 1.8e-5, 9.3e-6; the four ODE models (no
    active bound in their picks) 2e-10 and 7e-9 at most.  No instance is left out in any case."""
    ocp, P, opts = nonlinear_problem(name)
    solver = mpcx.nlpsol(name + "_bnd", "mi355x", ocp, {"ipopt": dict(opts, tol=1e-10)})
    lb, ub = sr.ocp_bounds(ocp)
    nom = solver.solve_batch(P)
    fd_check(solver, name, ocp, P, nom, np.tile(lb, (P.shape[0], 1)), np.tile(ub, (P.shape[0], 1)), {})


def fd_check(solver, name, ocp, P, nom, lb, ub, own):
    """the comparison of test 3 at the nominal solution nom under the bounds lb, ub (B, n_w); own: the bounds
    arguments of the sensitivity call ({}: the problem's own bounds)"""
    nx, B = ocp.nx, P.shape[0]
    assert np.all(nom["status"] <= 1), nom["status"]
    dlb, dub = seeded_directions(name, lb[0], ub[0], B, nx)
    s = solver.sens_bounds(P, nom, dlb, dub, **own)
    assert np.all(s["flag"] == 0), s["flag"]
    act0, same = [], np.ones(B, bool)
    for b in range(B):
        a, ok = sr.classify(nom["w"][b], nom["lam_x"][b], lb[b], ub[b], nx)
        if own:  # (bounds drawn in by the test: an instance that is not strictly complementary is left out)
            same[b] = ok
        else:
            assert ok, (name, b, "the nominal solution is not strictly complementary")
        act0.append(a)
    fd = {}
    for h in (1e-3, 1e-4):
        d = np.zeros((B, nom["w"].shape[1], 2))
        for j in range(2):
            side = []
            for sgn in (1.0, -1.0):
                lbj, ubj = lb + sgn * h * dlb[:, j], ub + sgn * h * dub[:, j]
                r = solver.solve_batch(P, w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"], lbw=lbj, ubw=ubj)
                for b in range(B):
                    a, ok = sr.classify(r["w"][b], r["lam_x"][b], lbj[b], ubj[b], nx)
                    same[b] &= bool(r["status"][b] <= 1 and ok and np.array_equal(a, act0[b]))
                side.append(r["w"])
            d[:, :, j] = (side[0] - side[1]) / (2 * h)
        fd[h] = d
    assert np.count_nonzero(~same) <= 1, (name, "instances whose active set changes", np.flatnonzero(~same))
    moved = 0.0
    for b in np.flatnonzero(same):
        spread = float(np.max(np.abs(fd[1e-3][b] - fd[1e-4][b])))
        err = float(np.max(np.abs(s["dw"][b] - 0.5 * (fd[1e-3][b] + fd[1e-4][b]))))
        print(f"{name} b={b}: {int(act0[b].sum())} active, FD spread {spread:.3e}, |GPU - FD| {err:.3e}, "
              f"|dw| {np.max(np.abs(s['dw'][b])):.3f}")
        assert err <= 4.0 * spread + 1e-6, (name, b)
        if act0[b].any():
            moved = max(moved, float(np.max(np.abs(s["dw"][b]))))
    # (the picks of the four ODE models have no active bound: there the check is of an O(mu) effect, and
    # test_nonlinear_with_drawn_in_bounds visits them with active ones)
    assert moved > 1e-3 or not any(act0[b].any() for b in np.flatnonzero(same))  # active bounds do move the solution
    return moved


def drawn_in_bounds(ocp, free_w, frac=0.8):
    """(lb, ub) (B, n_w): the problem's bounds with every input's box drawn in to `frac` of the instance's
    largest move of that input in the free solution, so that the bound is active at its largest moves"""
    nx, nu, N, B = ocp.nx, ocp.nu, ocp.N, free_w.shape[0]
    lb0, ub0 = sr.ocp_bounds(ocp)
    lb, ub = np.tile(lb0, (B, 1)), np.tile(ub0, (B, 1))
    top = frac * np.max(np.abs(free_w[:, nx:].reshape(B, N, nx + nu)[:, :, :nu]), axis=1)  # (B, nu)
    for k in range(N):
        iu = sr.iu_w(nx, nu, k)
        lb[:, iu], ub[:, iu] = np.maximum(lb[:, iu], -top), np.minimum(ub[:, iu], top)
    return lb, ub


@pytest.mark.parametrize("name", ["kin_bicycle_N10", "cartpole_N20", "path_bicycle_N20", "dyn_bicycle_N10"])
def test_nonlinear_with_drawn_in_bounds(mpcx, name):
    """3b. The four ODE models' picks have no active bound under the problems' own bounds, so tests 3 and 4
    see only the barrier's O(mu) there.  Here the same points get per-instance (B, n_w) bounds drawn in to
    0.8 of each instance's largest free move of every input, which makes bounds active (central differences
    are no reference at these points: the next-largest moves sit weakly on the bound, and every instance
    would be left out).  Checked: the dot-product identity of the reverse against the forward mode within
    its 64 x e_ref bound, and that a clearly active variable (sens_ref.classify) moves with its bound.
    Tolerance of the latter: its row reads Sigma (dw_i - dbound_i) + nu_i = 0 with Sigma = lam^2 / mu >=
    (1e-2)^2 / 1e-11 = 1e7 at the solver's tol = 1e-10 and |nu_i| the reduced curvature times |dw|, at most
    1e3 for these weights: 1e-4."""
    ocp, P, opts = nonlinear_problem(name)
    solver = mpcx.nlpsol(name + "_bnd2", "mi355x", ocp, {"ipopt": dict(opts, tol=1e-10)})
    free = solver.solve_batch(P)
    assert np.all(free["status"] <= 1), free["status"]
    lb, ub = drawn_in_bounds(ocp, free["w"])
    nom = solver.solve_batch(P, lbw=lb, ubw=ub)
    assert np.all(nom["status"] <= 1), nom["status"]
    B = P.shape[0]
    dlb, dub = seeded_directions(name, lb[0], ub[0], B, ocp.nx)
    g = np.random.default_rng(660 + NONLINEAR_CASES.index(name)).normal(size=(B, 2, nom["w"].shape[1]))
    s = solver.sens_bounds(P, nom, dlb, dub, lbw=lb, ubw=ub)
    v = solver.sens_bounds_vjp(P, nom, g, lbw=lb, ubw=ub)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    gap, bound = identity_gap(g, s["dw"], v["glbw"], v["gubw"], dlb, dub)
    n_act, worst = 0, 0.0
    for b in range(B):
        act, _ = sr.classify(nom["w"][b], nom["lam_x"][b], lb[b], ub[b], ocp.nx)
        n_act += int(act.sum())
        dbound = np.where((nom["lam_x"][b] < 0)[:, None], dlb[b].T, dub[b].T)
        if act.any():
            worst = max(worst, float(np.max(np.abs(s["dw"][b][act] - dbound[act]))))
    print(f"{name}: {n_act} clearly active bounds, |dw| {np.abs(s['dw']).max():.3g}, |g_lb|, |g_ub| "
          f"{np.abs(v['glbw']).max():.3g}, {np.abs(v['gubw']).max():.3g}, worst identity gap / bound "
          f"{np.max(gap / bound):.3e}, active variables off their bound's move by {worst:.3e}")
    assert np.all(gap <= bound) and worst <= 1e-4
    # the drawn-in bounds are felt (the cart-pole's multipliers stay below classify's 1e-2: none "clearly" active)
    assert n_act > 0 or name == "cartpole_N20"
    assert np.abs(s["dw"]).max() > 1e-3 and max(np.abs(v["glbw"]).max(), np.abs(v["gubw"]).max()) > 1e-3


# ------------------------------------------------------------------------------------------
# 4. reverse against forward: the dot-product identity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_dot_product_identity(mpcx, name):
    """4. <g, dw> = <g_lb, dlb> + <g_ub, dub> with dw the project's own sens_bounds at the same point, nx seeded
    directions and nx seeded cotangents, within the 64 x e_ref bound (identity_gap).  Measured on one MI355X,
    worst gap / bound: 1.1e-4 to 5.4e-4 (cart-pole QP 9e-15: no bound active)."""
    _, _, _, _, dlb, dub, s, g, v = linear_bounds_case(name)
    assert np.all(v["flag"] == 0) and v["glbw"].shape == g.shape and v["gubw"].shape == g.shape
    gap, bound = identity_gap(g, s["dw"], v["glbw"], v["gubw"], dlb, dub)
    print(f"{name}: worst identity gap {gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound)


@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_nonlinear_dot_product_identity(mpcx, name):
    """4. The same on all seven nonlinear models, two seeded directions and two seeded cotangents.  Measured on
    one MI355X, worst gap / bound: the three unicycle cases 1.5e-4 to 3.4e-4 (|dw| up to 9.8, |g_ub| up to 7.8);
    the four ODE models' picks have no active bound (|dw|, |g| <= 1e-6): 1e-13 and below."""
    ocp, P, opts = nonlinear_problem(name)
    solver = mpcx.nlpsol(name + "_bvjp", "mi355x", ocp, {"ipopt": opts})
    nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), nom["status"]
    B = P.shape[0]
    lb, ub = sr.ocp_bounds(ocp)
    dlb, dub = seeded_directions(name, lb, ub, B, ocp.nx)
    g = np.random.default_rng(650 + NONLINEAR_CASES.index(name)).normal(size=(B, 2, nom["w"].shape[1]))
    s, v = solver.sens_bounds(P, nom, dlb, dub), solver.sens_bounds_vjp(P, nom, g)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    gap, bound = identity_gap(g, s["dw"], v["glbw"], v["gubw"], dlb, dub)
    print(f"{name}: |dw| {np.abs(s['dw']).max():.3g}, |g_lb|, |g_ub| {np.abs(v['glbw']).max():.3g}, "
          f"{np.abs(v['gubw']).max():.3g}, worst identity gap {gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound)
    active = any(sr.classify(nom["w"][b], nom["lam_x"][b], lb, ub, ocp.nx)[0].any() for b in range(B))
    # (the picks of the four ODE models have no active bound: their gradients are the barrier's O(mu))
    assert max(np.abs(v["glbw"]).max(), np.abs(v["gubw"]).max()) > (1e-3 if active else 0.0)


# ------------------------------------------------------------------------------------------
# 5. exact properties
# ------------------------------------------------------------------------------------------
def exact_properties(solver, P, r, lb, ub, nx, seed, alone=None):
    """Zero directions / cotangents give zeros; entries on X_0 and on free bounds change nothing (NaN there
    is never read); column c of an (nx + 1)-column call (two launches) = that column alone; an instance
    alone = inside its batch (the instances `alone`, default all); glbw / gubw are exact zeros on X_0 and
    where there is no finite bound."""
    B, n_w = r["w"].shape
    rng = np.random.default_rng(seed)
    m = nx + 1
    dlb, dub, g = (rng.normal(size=(B, m, n_w)) for _ in range(3))
    s, v = solver.sens_bounds(P, r, dlb, dub), solver.sens_bounds_vjp(P, r, g)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    assert s["dw"].shape == (B, n_w, m) and v["glbw"].shape == (B, m, n_w) and v["gubw"].shape == (B, m, n_w)
    zero = np.zeros((B, 2, n_w))
    assert np.all(solver.sens_bounds(P, r, zero, zero)["dw"] == 0.0)
    vz = solver.sens_bounds_vjp(P, r, zero)
    assert np.all(vz["glbw"] == 0.0) and np.all(vz["gubw"] == 0.0)
    hl, hu = lb > -sr.INF_BOUND, ub < sr.INF_BOUND
    hl[:nx] = hu[:nx] = False
    junk = solver.sens_bounds(P, r, np.where(hl, dlb, np.nan), np.where(hu, dub, np.nan))
    assert bits(junk["dw"]) == bits(s["dw"])
    assert bits(solver.sens_bounds(P, r, dlb, None)["dw"]) == bits(solver.sens_bounds(P, r, dlb, 0.0 * dub)["dw"])
    assert bits(solver.sens_bounds(P, r, None, dub)["dw"]) == bits(solver.sens_bounds(P, r, 0.0 * dlb, dub)["dw"])
    assert np.all(v["glbw"][:, :, ~hl] == 0.0) and np.all(v["gubw"][:, :, ~hu] == 0.0)
    assert np.all(np.isfinite(v["glbw"])) and np.all(np.isfinite(v["gubw"]))
    first = solver.sens_bounds(P, r, dlb[:, :nx], dub[:, :nx]), solver.sens_bounds_vjp(P, r, g[:, :nx])
    assert bits(first[0]["dw"]) == bits(s["dw"][:, :, :nx])
    assert bits(first[1]["glbw"]) == bits(v["glbw"][:, :nx]) and bits(first[1]["gubw"]) == bits(v["gubw"][:, :nx])
    for c in range(m):
        one = solver.sens_bounds(P, r, dlb[:, c], dub[:, c])  # (B, n_w): a single direction
        assert one["dw"].shape == (B, n_w, 1) and bits(one["dw"][:, :, 0]) == bits(s["dw"][:, :, c]), c
        one = solver.sens_bounds_vjp(P, r, g[:, c])
        assert bits(one["glbw"][:, 0]) == bits(v["glbw"][:, c]) and bits(one["gubw"][:, 0]) == bits(v["gubw"][:, c]), c
    for b in range(B) if alone is None else alone:
        pt = point_of(r, slice(b, b + 1))
        solo = solver.sens_bounds(P[b:b + 1], pt, dlb[b:b + 1, :nx], dub[b:b + 1, :nx])
        assert bits(solo["dw"][0]) == bits(first[0]["dw"][b]) and solo["flag"][0] == 0, b
        solo = solver.sens_bounds_vjp(P[b:b + 1], pt, g[b:b + 1, :nx])
        assert bits(solo["glbw"][0]) == bits(first[1]["glbw"][b]) and bits(solo["gubw"][0]) == bits(first[1]["gubw"][b]), b
    return s, v


def test_exact_properties_unicycle(mpcx):
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("exact_bnd", "mi355x", ocp, {"ipopt": REF_OPTS})
    P = unicycle_P(5, 1)
    r = solver.solve_batch(P)
    lb, ub = sr.ocp_bounds(ocp)
    s, v = exact_properties(solver, P, r, lb, ub, 3, 31)
    assert np.max(np.abs(s["dw"])) > 1e-3 and max(np.abs(v["glbw"]).max(), np.abs(v["gubw"]).max()) > 1e-3
    with pytest.raises(ValueError):
        solver.sens_bounds(P, r, np.zeros((4, 3, 53)), None)
    with pytest.raises(ValueError):
        solver.sens_bounds(P, r, None, None)
    with pytest.raises(ValueError):
        solver.sens_bounds_vjp(P, r, np.zeros((5, 3, 52)))


@pytest.mark.parametrize("name", ["padded_dint_N8", "ltv_N40"])
def test_exact_properties_linear(mpcx, name):
    lin, P, r, solver, _, _, _, _, _ = linear_bounds_case(name)
    lb, ub = sr.ocp_bounds(lin)
    # (a schedule per instance, ltv_N40: a batch of one reads the first row, so instance 0 is the one alone)
    exact_properties(solver, P, r, lb, ub, lin.nx, 32, alone=None if lin.tab.ndim == 1 else [0])


def test_per_instance_bounds_equal_shared_ones(mpcx):
    """(B, n_w) bounds installed for the call give the bits of the same bounds passed as one shared row, and
    whatever was installed before is put back."""
    lin, P, r, solver, dlb, dub, s, g, v = linear_bounds_case("lin4x2_N12")
    lb, ub = sr.ocp_bounds(lin)
    B = P.shape[0]
    before = solver._dev_bounds
    sp_ = solver.sens_bounds(P, r, dlb, dub, lbw=np.tile(lb, (B, 1)), ubw=np.tile(ub, (B, 1)))
    vp = solver.sens_bounds_vjp(P, r, g, lbw=np.tile(lb, (B, 1)), ubw=np.tile(ub, (B, 1)))
    assert solver._dev_bounds is before
    assert bits(sp_["dw"]) == bits(s["dw"]) and bits(vp["glbw"]) == bits(v["glbw"]) and bits(vp["gubw"]) == bits(v["gubw"])
    sh = solver.sens_bounds(P, r, dlb, dub, lbw=lb, ubw=ub)
    assert bits(sh["dw"]) == bits(s["dw"])


@pytest.mark.parametrize("name", ["unicycle_N10", "padded_dint_N8"])
def test_device_loop_equals_host_call(mpcx, name):
    """DeviceLoop.sens_bounds / sens_bounds_vjp after solve() against the host calls on the loop's tensors
    copied back, bit for bit; every entry of glbw / gubw is written (outputs pre-filled with 7); the point=
    override on a saved copy gives the same bits after the loop has moved on."""
    import torch
    from mpcx.device import DeviceLoop

    if name == "unicycle_N10":
        ocp, P = mpcx.unicycle_point_to_point(N=10), unicycle_P(5, 1)
        solver = mpcx.nlpsol(name + "_bl", "mi355x", ocp, {"ipopt": REF_OPTS})
        n_w = 53
    else:
        ocp, P = linear_problem(name)
        solver = mpcx.nlpsol(name + "_bl", "mi355x", ocp, {"ipopt": {"max_iter": 300}})
        n_w = ocp.n_w_ms
    pd = solver._pad
    B, m = P.shape[0], ocp.nx
    rng = np.random.default_rng(33)
    dlb, dub, g = (rng.normal(size=(B, m, n_w)) for _ in range(3))
    k = lambda a: a if pd is None else pd.scatter(a.reshape(B * m, -1), pd.w_idx, pd.n_w_pad).reshape(B, m, -1)  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(k(a))).to("cuda:0")  # noqa: E731
    d_dlb, d_dub, d_g = dev(dlb), dev(dub), dev(g)
    loop = DeviceLoop(solver, P, device="cuda:0")
    loop.solve()
    nwk = loop.w.shape[1]
    gl_out, gu_out = (torch.full((B, m, nwk), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
    dw, flag = loop.sens_bounds(d_dlb, d_dub)
    gl, gu, vflag = loop.sens_bounds_vjp(d_g, glbw_out=gl_out, gubw_out=gu_out)
    only_l = loop.sens_bounds(d_dlb, None)[0]
    saved = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    torch.cuda.synchronize()
    assert gl is gl_out and gu is gu_out and not bool((gl == 7.0).any()) and not bool((gu == 7.0).any())
    host = {k_: t.cpu().numpy() for k_, t in (("P", loop.P), ("w", loop.w), ("lam_g", loop.lam), ("lam_x", loop.lamx))}
    dw_np, gl_np, gu_np = dw.cpu().numpy(), gl.cpu().numpy(), gu.cpu().numpy()
    if pd is not None:  # the loop's tensors hold the kernel's padded layout
        assert not gl_np[:, :, np.setdiff1d(np.arange(nwk), pd.w_idx)].any()  # the pad states: exact zeros
        host = {"P": host["P"][:, pd.p_idx], "w": host["w"][:, pd.w_idx], "lam_g": host["lam_g"][:, pd.g_idx],
                "lam_x": host["lam_x"][:, pd.w_idx]}
        dw_np, gl_np, gu_np = dw_np[:, pd.w_idx], gl_np[:, :, pd.w_idx], gu_np[:, :, pd.w_idx]
    s, v = solver.sens_bounds(host["P"], host, dlb, dub), solver.sens_bounds_vjp(host["P"], host, g)
    assert np.all(s["flag"] == 0) and bits(flag.cpu().numpy()) == bits(s["flag"]) == bits(vflag.cpu().numpy())
    assert bits(dw_np) == bits(s["dw"]) and bits(gl_np) == bits(v["glbw"]) and bits(gu_np) == bits(v["gubw"])
    assert bits(only_l.cpu().numpy()) == bits(loop.sens_bounds(d_dlb, torch.zeros_like(d_dub))[0].cpu().numpy())
    loop.step()  # the resident point moves on
    loop.solve()
    again = loop.sens_bounds(d_dlb, d_dub, point=saved)[0], loop.sens_bounds_vjp(d_g, point=saved)[0]
    moved = loop.sens_bounds(d_dlb, d_dub)[0]
    torch.cuda.synchronize()
    assert bits(again[0].cpu().numpy()) == bits(dw.cpu().numpy()) and bits(again[1].cpu().numpy()) == bits(gl.cpu().numpy())
    assert bits(moved.cpu().numpy()) != bits(dw.cpu().numpy())
    with pytest.raises(ValueError):
        loop.sens_bounds_vjp(d_g, glbw_out=gl_out[:, :1])
    with pytest.raises(ValueError):
        loop.sens_bounds(torch.zeros((B, loop._knx + 1, nwk), dtype=torch.float64, device="cuda:0"), None)
    with pytest.raises(ValueError):
        loop.sens_bounds(None, None)


# ------------------------------------------------------------------------------------------
# 6. irregular instances: ordinary statuses, nothing faults
# ------------------------------------------------------------------------------------------
def assert_only_irregular(s, v, bad, regular=None):
    for b in range(s["flag"].shape[0]):
        if b == bad:
            assert s["flag"][b] == 1 and v["flag"][b] == 1
            assert np.all(np.isnan(s["dw"][b])) and np.all(np.isnan(v["glbw"][b])) and np.all(np.isnan(v["gubw"][b]))
        else:
            assert s["flag"][b] == 0 and v["flag"][b] == 0
            assert np.all(np.isfinite(s["dw"][b])) and np.all(np.isfinite(v["glbw"][b])) and np.all(np.isfinite(v["gubw"][b]))
            if regular is not None:  # the neighbours keep their bits
                assert bits(s["dw"][b]) == bits(regular[0]["dw"][b]), b
                assert bits(v["glbw"][b]) == bits(regular[1]["glbw"][b]) and bits(v["gubw"][b]) == bits(regular[1]["gubw"][b]), b


def test_variable_on_its_bound_is_flagged(mpcx):
    lin, P, r, solver, dlb, dub, s, g, v = linear_bounds_case("padded_dint_N8")
    w = r["w"].copy()
    w[2, lin.nx + (lin.nx + lin.nu) * 3] = 1.0  # U_3 of instance 2 placed on its upper bound
    pt = {"w": w, "lam_g": r["lam_g"], "lam_x": r["lam_x"]}
    assert_only_irregular(solver.sens_bounds(P, pt, dlb, dub), solver.sens_bounds_vjp(P, pt, g), 2, (s, v))


def test_indefinite_stage_is_flagged(mpcx):
    """A negative input weight on the last stage of instance 1 of 3 (tests/test_gpu_sens.py's case)."""
    from mpcx import lti

    rng = np.random.default_rng(11)
    nx, nu, N, B = 4, 1, 20, 3
    A = np.eye(nx) + 0.05 * rng.normal(size=(nx, nx))
    Bm = rng.normal(size=(nx, nu)) + 1.0
    W = np.zeros((2, nx + nu, nx + nu))
    W[:, :nx, :nx] = 5.0 * np.eye(nx)
    W[0, nx, nx] = 0.5
    W[1, nx, nx] = -0.05
    tab = np.zeros((B, N), np.int32)
    tab[1, -1] = 1
    lin = lti.LinearOCP(N=N, A=np.stack([A, A]), B=np.stack([Bm, Bm]), W=W, tab=tab, u_lb=(-1.0,), u_ub=(1.0,))
    solver = mpcx.nlpsol("indef_bnd", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    P = lin.params(rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    point = {"w": np.zeros((B, lin.n_w_ms)), "lam_g": np.zeros((B, lin.n_g_ms)), "lam_x": np.zeros((B, lin.n_w_ms))}
    d, g = rng.normal(size=(B, 2, lin.n_w_ms)), rng.normal(size=(B, 2, lin.n_w_ms))
    assert_only_irregular(solver.sens_bounds(P, point, d, -d), solver.sens_bounds_vjp(P, point, g), 1)


# ------------------------------------------------------------------------------------------
# 7. refusals: MPCX_EINVAL with a message, nothing launched
# ------------------------------------------------------------------------------------------
def test_refusals(mpcx):
    """m = 0 and m = nx + 1, N = 64, null pointers, B < 1, a null handle, on all four entry points; the
    path-frame bicycle (model 7 of the registry's count) is accepted."""
    import torch
    from mpcx import _lib, ode

    lib = _lib.load()
    EINVAL = -1

    def host_call(solver, vjp, B=2, m=1, n_null=()):
        h = solver._h
        n, mm = max(B, 1), max(m, 1)
        arr = [np.zeros((n, h.n_p)), np.zeros((n, h.n_w)), np.zeros((n, h.n_g)), np.zeros((n, h.n_w)),
               np.zeros((n, mm, h.n_w)), np.zeros((n, mm, h.n_w)), np.full((n, h.n_w, mm), 7.0)]
        a = [None if i in n_null else _lib.dptr(x) for i, x in enumerate(arr)]
        if vjp:  # gw = arr[4]; glbw, gubw = arr[5], arr[6]
            arr[5][:] = 7.0
            rc = lib.mpcx_sens_bounds_vjp(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], m, a[5], a[6], None)
            assert np.all(arr[5] == 7.0)
        else:  # dlbw, dubw = arr[4], arr[5]; dw = arr[6]
            rc = lib.mpcx_sens_bounds(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], a[5], m, a[6], None)
        assert rc != 0 and np.all(arr[6] == 7.0)
        return rc, lib.mpcx_last_error().decode()

    solver = mpcx.nlpsol("ok_bnd", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    long = mpcx.nlpsol("n64_bnd", "mi355x", mpcx.unicycle_point_to_point(N=64), {"ipopt": REF_OPTS})
    buf = torch.zeros(2 * long._h.n_w * 4, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())

    def dev_call(h, vjp, B=2, m=1, lam_g=p, a=p, b=p, c=p):
        if vjp:
            rc = lib.mpcx_sens_bounds_vjp_dev(h.ptr if h else None, B, p, p, lam_g, p, a, m, b, c, None, None)
        else:
            rc = lib.mpcx_sens_bounds_dev(h.ptr if h else None, B, p, p, lam_g, p, a, b, m, c, None, None)
        return rc, lib.mpcx_last_error().decode()

    for vjp in (False, True):
        who = "sens_bounds_vjp" if vjp else "sens_bounds:"
        for call, ok, n64 in ((host_call, solver, long), (dev_call, solver._h, long._h)):
            for m in (0, 4):
                rc, msg = call(ok, vjp, m=m)
                assert rc == EINVAL and "between 1 and nx" in msg and who in msg, (m, msg)
            for B in (0, -3):
                rc, msg = call(ok, vjp, B=B)
                assert rc == EINVAL and "B must be >= 1" in msg
            rc, msg = call(n64, vjp)
            assert rc == EINVAL and "N >= 64" in msg
        for i in range(7):  # P, w, lam_g, lam_x and the three direction / cotangent / output arrays
            rc, msg = host_call(solver, vjp, n_null=(i,))
            assert rc == EINVAL and "required" in msg, i
        for kw in ({"lam_g": None}, {"a": None}, {"b": None}, {"c": None}):
            rc, msg = dev_call(solver._h, vjp, **kw)
            assert rc == EINVAL and "required" in msg, kw
        rc, msg = dev_call(None, vjp)
        assert rc == EINVAL and "null handle" in msg
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched
    # the path-frame bicycle, which sens_p / sens_vjp refuse, is accepted
    ocp, P, opts = nonlinear_problem("path_bicycle_N20")
    path = mpcx.nlpsol("path_bnd", "mi355x", ocp, {"ipopt": opts})
    r = path.solve_batch(P)
    d = np.ones((P.shape[0], 1, r["w"].shape[1]))
    assert np.all(path.sens_bounds(P, r, d, -d)["flag"] == 0) and np.all(path.sens_bounds_vjp(P, r, d)["flag"] == 0)


# ------------------------------------------------------------------------------------------
# 8. autograd
# ------------------------------------------------------------------------------------------
def test_autograd_bounds(mpcx):
    """solve_differentiable with (B, n_w) bounds on unicycle_N10: lbw.grad / ubw.grad equal a direct
    DeviceLoop.sens_bounds_vjp launch at the saved point bit for bit and P.grad equals sens_vjp's; the backward
    differentiates at the forward's bounds also after the loop's bounds were changed, and puts the changed
    ones back; the call without bounds is MPCFunction's, bit for bit what it was."""
    import torch
    from mpcx.autograd import MPCFunction, solve_differentiable
    from mpcx.device import DeviceLoop

    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("autograd_bnd", "mi355x", ocp, {"ipopt": REF_OPTS})
    P0 = unicycle_P(5, 1)
    B, nx, nu, n_w = 5, 3, 2, 53
    lb0, ub0 = sr.ocp_bounds(ocp)
    t64 = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device="cuda:0", requires_grad=grad)  # noqa: E731
    u_t = t64(np.random.default_rng(17).uniform(-0.5, 0.5, (B, nu)))
    grads = []
    for change_bounds in (False, True):
        loop = DeviceLoop(solver, P0, device="cuda:0")
        P, lbw, ubw = t64(P0, True), t64(np.tile(lb0, (B, 1)), True), t64(np.tile(ub0, (B, 1)), True)
        w = solve_differentiable(loop, P, lbw=lbw, ubw=ubw)
        assert w.shape == (B, n_w) and w.requires_grad
        point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
        gw = torch.zeros((B, 1, n_w), dtype=torch.float64, device="cuda:0")
        gw[:, 0, nx:nx + nu] = (w[:, nx:nx + nu] - u_t).detach()
        direct = loop.sens_bounds_vjp(gw, point=point), loop.sens_vjp(gw, point=point)
        other = None
        if change_bounds:  # looser input bounds installed after the forward: the backward must not use them
            loop.set_bounds(t64(np.tile(lb0, (B, 1)) - 0.25), t64(np.tile(ub0, (B, 1)) + 0.25))
            other = solver._dev_bounds
        (0.5 * ((w[:, nx:nx + nu] - u_t) ** 2).sum()).backward()
        torch.cuda.synchronize()
        assert solver._dev_bounds is other or not change_bounds
        assert int(direct[0][2].sum()) == 0
        assert bits(lbw.grad.cpu().numpy()) == bits(direct[0][0][:, 0].cpu().numpy())
        assert bits(ubw.grad.cpu().numpy()) == bits(direct[0][1][:, 0].cpu().numpy())
        assert bits(P.grad.cpu().numpy()) == bits(direct[1][0][:, 0].cpu().numpy())
        grads.append((lbw.grad.cpu().numpy(), ubw.grad.cpu().numpy()))
        solver._install_bounds(None)
    assert bits(grads[0][0]) == bits(grads[1][0]) and bits(grads[0][1]) == bits(grads[1][1])
    assert max(np.abs(grads[0][0]).max(), np.abs(grads[0][1]).max()) > 1e-3
    assert not grads[0][0][:, :nx].any() and not grads[0][0][:, lb0 < -sr.INF_BOUND].any()
    # bounds gradients alone: no sens_vjp launch is needed, P gets no gradient
    loop = DeviceLoop(solver, P0, device="cuda:0")
    P, lbw, ubw = t64(P0), t64(np.tile(lb0, (B, 1)), True), t64(np.tile(ub0, (B, 1)))
    w = solve_differentiable(loop, P, lbw=lbw, ubw=ubw)
    (0.5 * ((w[:, nx:nx + nu] - u_t) ** 2).sum()).backward()
    assert bits(lbw.grad.cpu().numpy()) == bits(grads[0][0]) and ubw.grad is None and P.grad is None
    solver._install_bounds(None)
    # without bounds: the MPCFunction path, unchanged
    loop = DeviceLoop(solver, P0, device="cuda:0")
    P = t64(P0, True)
    w = solve_differentiable(loop, P)
    assert type(w.grad_fn).__name__ == MPCFunction.__name__ + "Backward"
    point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    (0.5 * ((w[:, nx:nx + nu] - u_t) ** 2).sum()).backward()
    gw = torch.zeros((B, 1, n_w), dtype=torch.float64, device="cuda:0")
    gw[:, 0, nx:nx + nu] = (w[:, nx:nx + nu] - u_t).detach()
    assert bits(P.grad.cpu().numpy()) == bits(loop.sens_vjp(gw, point=point)[0][:, 0].cpu().numpy())
    with pytest.raises(ValueError):
        solve_differentiable(loop, P, lbw=lbw)


def test_autograd_bounds_path_bicycle(mpcx):
    """Model 7, which has no sens_vjp: gradients with respect to the bounds alone.  The bounds handed in are
    the problem's with the input bounds drawn in to 0.8 of each instance's largest free move, so that some
    are active and the gradients are O(1)."""
    import torch
    from mpcx.autograd import solve_differentiable
    from mpcx.device import DeviceLoop

    ocp, P0, opts = nonlinear_problem("path_bicycle_N20")
    solver = mpcx.nlpsol("autograd_path", "mi355x", ocp, {"ipopt": opts})
    B = P0.shape[0]
    free = solver.solve_batch(P0)
    assert np.all(free["status"] <= 1)
    lb, ub = drawn_in_bounds(ocp, free["w"])
    t64 = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device="cuda:0", requires_grad=grad)  # noqa: E731
    loop = DeviceLoop(solver, P0, device="cuda:0")
    lbw, ubw = t64(lb, True), t64(ub, True)
    w = solve_differentiable(loop, t64(P0), lbw=lbw, ubw=ubw)
    point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    w.sum().backward()
    gl, gu, flag = loop.sens_bounds_vjp(torch.ones((B, 1, w.shape[1]), dtype=torch.float64, device="cuda:0"), point=point)
    torch.cuda.synchronize()
    assert int(flag.sum()) == 0 and int(loop.status.max()) <= 1
    assert bits(lbw.grad.cpu().numpy()) == bits(gl[:, 0].cpu().numpy())
    assert bits(ubw.grad.cpu().numpy()) == bits(gu[:, 0].cpu().numpy())
    assert max(float(lbw.grad.abs().max()), float(ubw.grad.abs().max())) > 1e-3
    solver._install_bounds(None)
