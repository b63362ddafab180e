"""GPU tests of the sensitivities of the MPC solution to the cost weights (mpcx_sens_weights[_vjp][_dev],
mpcx_set_weights, Solver.sens_weights / sens_weights_vjp / set_weights, DeviceLoop.sens_weights /
sens_weights_vjp, mpcx.autograd with Q=, R=; csrc/sens.h sens_wt_kernel, sens_wt_vjp_kernel).

References: tests/helpers/sens_weights_ref.py -- the kernel's two rounds restated in long double from the GPU's
own point -- central differences of the solver itself on problems with perturbed weights for the nonlinear
models, and the project's forward mode for the reverse one, through the dot-product identity
<g, dw> = sum_k <gWk_k, dW_k>.  Cases are those of tests/test_gpu_sens.py, test_gpu_sens_p.py and
test_gpu_sens_bounds.py (their constructors and cached solves are imported)."""
import ctypes
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sens_ref as sr  # noqa: E402
import sens_weights_ref as sw  # noqa: E402
from test_gpu_sens import (LINEAR_CASES, NONLINEAR_CASES, REF_OPTS, linear_case, linear_problem,  # noqa: E402
                           nonlinear_problem, unicycle_P)
from test_gpu_sens_bounds import edge_case  # noqa: E402
from test_gpu_sens_p import nonlinear_p_problem  # noqa: E402

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


def residuals(lin, Pb, wb, dtype=LD):
    """e (N, nz) of a LinearOCP's instance: z_k - zr_k with z_0 = (x0 of P, U_0), as the kernel evaluates stage 0"""
    nx, nu, N = lin.nx, lin.nu, lin.N
    wb, Pb = np.asarray(wb, dtype), np.asarray(Pb, dtype)
    z = np.stack([np.concatenate([Pb[:nx] if k == 0 else wb[sr.ix_w(nx, nu, k)], wb[sr.iu_w(nx, nu, k)]])
                  for k in range(N)])
    return z - Pb[nx:].reshape(N, nx + nu)


def restated(lin, P, r, b, lb, ub, dWp, g):
    """(dw (n_w, m), gWk (m, N, nh)) of the kernels' two rounds in long double at the GPU's own point of
    instance b: dWp (m, N, nh) packed directions, g (m, n_w) cotangents"""
    A, Bm, H = sr.linear_operands(lin, b)
    Sig = sr.sigma_of(r["w"][b], r["lam_x"][b], lb, ub, lin.nx, lin.nu, LD)
    e = residuals(lin, P[b], r["w"][b])
    dw = sw.reference(A, Bm, H, Sig, sw.packed_rhs(np.asarray(dWp, LD), e))
    zt = sw.reference_z(A, Bm, H, Sig, np.asarray(g.T, LD))
    return dw, sw.packed_vjp(zt, e)


def identity_gap(g, dw, gk, d):
    """(|<g, dw> - sum_k <gWk_k, dW_k>|, bound) per (instance, cotangent, direction), the form of
    tests/test_gpu_sens_bounds.py's identity_gap with the yardsticks of the weights: g (B, mg, n_w),
    dw (B, n_w, md), gk (B, mg, N, n_wt), d (B, md, N, n_wt)."""
    lhs = np.einsum("bci,bij->bcj", g, dw)
    rhs = np.einsum("bckn,bjkn->bcj", gk, d)
    big = lambda v: np.maximum(1.0, np.abs(v))  # noqa: E731
    bound = (64.0 * sw.e_ref_w() * np.einsum("bci,bij->bcj", np.abs(g), big(dw))
             + 64.0 * sw.e_ref_wvjp() * np.einsum("bckn,bjkn->bcj", big(gk), np.abs(d)))
    return np.abs(lhs - rhs), bound


def sum_gap(gs, gk):
    """(|gW - sum_k gWk_k|, bound): the stage sum of the kernel (gsum) against NumPy's, in the form of the
    reverse half of identity_gap with unit directions"""
    return np.abs(gs - gk.sum(axis=2)), 64.0 * sw.e_ref_wvjp() * np.maximum(1.0, np.abs(gk)).sum(axis=2)


def tab_of(lin, B):
    tab = np.asarray(lin.tab)
    return np.broadcast_to(tab[None, :] if tab.ndim == 1 else tab, (B, lin.N))


# ------------------------------------------------------------------------------------------
# 1. linear cases: test_gpu_sens.py's solves, shared, never modified
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_weights_case(name):
    """(lin, P, solve result, solver, dW (B, nx, N, nh) packed per-stage directions: column 0 the stage's own
    table W, the others seeded normal, sens_weights result, g (B, nx, n_w) seeded normal, sens_weights_vjp result)"""
    from mpcx import lti

    lin, P, r, _, solver = linear_case(name)
    B, nz = P.shape[0], lin.nx + lin.nu
    rng = np.random.default_rng(900 + LINEAR_CASES.index(name))
    dW = rng.normal(size=(B, lin.nx, lin.N, nz * (nz + 1) // 2))
    dW[:, 0] = lti.pack_sym(lin.W)[tab_of(lin, B)]
    g = rng.normal(size=(B, lin.nx, lin.n_w_ms))
    s = solver.sens_weights(P, r, dW=dW)
    v = solver.sens_weights_vjp(P, r, g)
    for a in (dW, g, *s.values(), *v.values()):
        a.setflags(write=False)
    return lin, P, r, solver, dW, s, g, v


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_restatement(mpcx, name):
    """1. Forward and reverse kernels against their two rounds restated in long double at the same point and
    tables: nx packed per-stage directions (column 0 is dW = W itself, the others seeded normal, off-diagonals
    included) and nx seeded normal cotangents: 64 x e_ref_w and 64 x e_ref_wvjp relative to max(1, |entry|)
    (e_ref_w = 4.3e-15, e_ref_wvjp = 3.7e-15: 2.8e-13 and 2.4e-13).  Measured on one MI355X, forward / reverse:
    padded_dint_N8 4.3e-16 / 2.1e-16, lin4x2_N12 1.4e-16 / 1.6e-16, ltv_N40 2.0e-16 / 1.1e-16, cartpole_qp_N50
    1.7e-14 / 2.2e-14 (|dw| up to 1e6 over its unstable open loop)."""
    lin, P, r, _, dW, s, g, v = linear_weights_case(name)
    B, nz = P.shape[0], lin.nx + lin.nu
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    assert s["dw"].shape == (B, lin.n_w_ms, lin.nx) and v["gWk"].shape == (B, lin.nx, lin.N, nz * (nz + 1) // 2)
    lb, ub = sr.ocp_bounds(lin)
    wf = wr = 0.0
    for b in range(B):
        dw, gk = restated(lin, P, r, b, lb, ub, dW[b], g[b])
        wf, wr = max(wf, sr.rel_err(s["dw"][b], dw)), max(wr, sr.rel_err(v["gWk"][b], gk))
        assert not s["dw"][b, :lin.nx].any()  # dX_0 = 0, exactly
    tf, tr = 64.0 * sw.e_ref_w(), 64.0 * sw.e_ref_wvjp()
    print(f"{name}: |dw| {np.abs(s['dw']).max():.3g}, |gWk| {np.abs(v['gWk']).max():.3g}; worst error against the "
          f"long-double restatement: forward {wf:.3e} (tolerance {tf:.3e}), reverse {wr:.3e} (tolerance {tr:.3e})")
    assert wf <= tf and wr <= tr
    assert np.abs(s["dw"]).max() > 1e-3 and np.abs(v["gWk"]).max() > 1e-3
    # gW: the stages' rows summed per table through the instance's schedule
    tab = tab_of(lin, B)
    ref = np.zeros_like(v["gW"])
    for b in range(B):
        for k in range(lin.N):
            ref[b, :, tab[b, k]] += v["gWk"][b, :, k]
    assert v["gW"].shape == (B, lin.nx, lin.n_tab, v["gWk"].shape[3]) and np.allclose(v["gW"], ref, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------
# 2. edge shapes: stage N - 1 on the last stage lane of its group
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [15, 31, 63])
def test_edge_shapes_against_the_restatement(mpcx, N):
    """2. N = 15, 31, 63 (tests/test_gpu_sens_bounds.py's edge_case: B = 5, per-instance bounds with a state
    bound at node N): node N - 1's weight row is read and written by lane G - 2, node N on lane G - 1 has
    none.  Forward and reverse against the long-double restatement, and the identity.  Measured on one MI355X,
    N = 15 / 31 / 63, forward / reverse: 1.4e-16 / 1.3e-16, 2.0e-16 / 2.3e-16, 2.0e-16 / 1.9e-16; identity gap /
    bound 9.2e-5, 6.0e-5, 1.4e-4."""
    lin, P, lb, ub, r, solver = edge_case(N)
    B, nz = P.shape[0], lin.nx + lin.nu
    rng = np.random.default_rng(950 + N)
    dW = rng.normal(size=(B, lin.nx, N, nz * (nz + 1) // 2))
    g = rng.normal(size=(B, lin.nx, lin.n_w_ms))
    s = solver.sens_weights(P, r, dW=dW, lbw=lb, ubw=ub)
    v = solver.sens_weights_vjp(P, r, g, lbw=lb, ubw=ub)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    wf = wr = 0.0
    for b in range(B):
        dw, gk = restated(lin, P, r, b, lb[b], ub[b], dW[b], g[b])
        wf, wr = max(wf, sr.rel_err(s["dw"][b], dw)), max(wr, sr.rel_err(v["gWk"][b], gk))
    gap, bound = identity_gap(g, s["dw"], v["gWk"], dW)
    print(f"N={N}: worst error against the long-double restatement: forward {wf:.3e}, reverse {wr:.3e}; identity gap "
          f"{gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert wf <= 64.0 * sw.e_ref_w() and wr <= 64.0 * sw.e_ref_wvjp()
    assert np.all(gap <= bound)
    assert np.abs(v["gWk"][:, :, N - 1]).max() > 1e-6  # the last stage's row is written


# ------------------------------------------------------------------------------------------
# 3. reverse against forward: the dot-product identity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_dot_product_identity(mpcx, name):
    """3. <g, dw> = sum_k <gWk_k, dW_k> with dw the project's own sens_weights at the same point, per-stage
    directions, within the 64 x e_ref bound (identity_gap).  Measured on one MI355X, worst gap / bound: 2.1e-5 to
    4.2e-4, cart-pole QP 2.5e-3."""
    _, _, _, _, dW, s, g, v = linear_weights_case(name)
    gap, bound = identity_gap(g, s["dw"], v["gWk"], dW)
    print(f"{name}: worst identity gap {gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound)


IDENTITY_CASES = NONLINEAR_CASES + ("unicycle_tracking_N10",)


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_nonlinear_dot_product_identity(mpcx, name):
    """3. The same on all seven nonlinear cases (the quadrature-cost unicycle in its three units, the four ODE
    models, the path-frame bicycle among them) and the node-cost unicycle: two seeded per-stage directions of
    (Q, R) and two seeded cotangents.  gQ, gR equal the sums of gQk, gRk over the stages within the reverse
    half of the bound.  Measured on one MI355X, worst gap / bound 9.9e-6 (6-state bicycle) to 7.9e-4 (cart-pole,
    |dw| 5e5); the stage sum 4.7e-5 to 1.2e-3 of its bound."""
    ocp, P, opts = nonlinear_p_problem(name)
    solver = mpcx.nlpsol(name + "_wvjp", "mi355x", ocp, {"ipopt": opts})
    nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), nom["status"]
    B, nx, nu, N = P.shape[0], ocp.nx, ocp.nu, ocp.N
    rng = np.random.default_rng(960 + IDENTITY_CASES.index(name))
    dQ, dR = rng.normal(size=(B, 2, N, nx)), rng.normal(size=(B, 2, N, nu))
    g = rng.normal(size=(B, 2, nom["w"].shape[1]))
    s, v = solver.sens_weights(P, nom, dQ=dQ, dR=dR), solver.sens_weights_vjp(P, nom, g)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    gk, d = np.concatenate([v["gQk"], v["gRk"]], axis=3), np.concatenate([dQ, dR], axis=3)
    gap, bound = identity_gap(g, s["dw"], gk, d)
    sg, sb_ = sum_gap(np.concatenate([v["gQ"], v["gR"]], axis=2), gk)
    print(f"{name}: |dw| {np.abs(s['dw']).max():.3g}, |gQk|, |gRk| {np.abs(v['gQk']).max():.3g}, "
          f"{np.abs(v['gRk']).max():.3g}, worst identity gap {gap.max():.3e}, worst gap / bound "
          f"{np.max(gap / bound):.3e}; stage sum off by {sg.max():.3e} (worst / bound {np.max(sg / sb_):.3e})")
    assert np.all(gap <= bound) and np.all(sg <= sb_)
    assert np.abs(s["dw"]).max() > 1e-3 and np.abs(gk).max() > 1e-3
    assert not s["dw"][:, :nx].any()
    if ocp.cost == "node":  # X~_0 = 0: stage 0's state weights get an exact zero
        assert not v["gQk"][:, :, 0].any()


# ------------------------------------------------------------------------------------------
# 4. nonlinear models against central differences of the solver itself on perturbed weights
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_nonlinear_against_finite_differences(mpcx, name):
    """4. dw against central differences of solves of dataclasses.replace(ocp, Q = Q +- h dQ, R = R +- h dR), a
    new solver each, warm-started from the nominal solution, at h = 1e-3 and 1e-4 with the directions relative
    to each weight: column 0 dQ = Q xi, dR = R xi with xi seeded normal, column 1 dQ = Q, dR = R (the whole
    objective scaled: what moves is the barrier's balance against it).  The solvers run at tol = 1e-10, for
    the reason tests/test_gpu_sens_bounds.py records.  Tolerance 4 x the spread of the two estimates + 1e-6
    against their mean.  So that the spread cannot hide a failure: an instance whose active set changes under
    +- h is left out, at most one per case; every instance kept has spread <= 1e-3 max(1, max|dw|); each case
    shows max|dw| > 1e-3 on the seeded column.  Spread and error are printed per instance.  Measured on one
    MI355X, worst instance of each case (spread, |GPU - FD|): unicycle_N10 1.2e-6, 6.1e-7; unicycle_bounded_N10
    2.8e-8, 1.4e-8; unicycle_N30 3.0e-7, 1.5e-7; kin_bicycle_N10 7.0e-7, 3.6e-7; cartpole_N20 5.4e-6, 2.8e-6
    (|dw| 19.8); path_bicycle_N20 1.8e-7, 9.4e-8; dyn_bicycle_N10 1.5e-6, 7.6e-7.  No instance is left out."""
    ocp, P, opts = nonlinear_problem(name)
    o = {"ipopt": dict(opts, tol=1e-10)}
    solver = mpcx.nlpsol(name + "_wt", "mi355x", ocp, o)
    nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), nom["status"]
    B, nx, nu = P.shape[0], ocp.nx, ocp.nu
    Q, R = np.array(ocp.Q, float)[:nx], np.array(ocp.R, float)[:nu]
    rng = np.random.default_rng(970 + NONLINEAR_CASES.index(name))
    dQ = np.stack([Q * rng.normal(size=nx), Q])
    dR = np.stack([R * rng.normal(size=nu), R])
    s = solver.sens_weights(P, nom, dQ=np.tile(dQ, (B, 1, 1)), dR=np.tile(dR, (B, 1, 1)))
    assert np.all(s["flag"] == 0), s["flag"]
    lb, ub = sr.ocp_bounds(ocp)
    act0, same = [], np.ones(B, bool)
    for b in range(B):
        a, ok = sr.classify(nom["w"][b], nom["lam_x"][b], lb, ub, nx)
        assert ok, (name, b, "the nominal solution is not strictly complementary")
        act0.append(a)
    fd = {}
    for h in (1e-3, 1e-4):
        d = np.zeros((B, nom["w"].shape[1], 2))
        for j in range(2):
            side = []
            for sgn in (1.0, -1.0):
                moved = dataclasses.replace(ocp, Q=tuple(Q + sgn * h * dQ[j]), R=tuple(R + sgn * h * dR[j]))
                r = mpcx.nlpsol(name + "_wt_fd", "mi355x", moved, o).solve_batch(
                    P, w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"])
                for b in range(B):
                    a, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, nx)
                    same[b] &= bool(r["status"][b] <= 1 and ok and np.array_equal(a, act0[b]))
                side.append(r["w"])
            d[:, :, j] = (side[0] - side[1]) / (2 * h)
        fd[h] = d
    assert np.count_nonzero(~same) <= 1, (name, "instances whose active set changes", np.flatnonzero(~same))
    seeded = 0.0
    for b in np.flatnonzero(same):
        spread = float(np.max(np.abs(fd[1e-3][b] - fd[1e-4][b])))
        err = float(np.max(np.abs(s["dw"][b] - 0.5 * (fd[1e-3][b] + fd[1e-4][b]))))
        top = float(np.max(np.abs(s["dw"][b])))
        print(f"{name} b={b}: {int(act0[b].sum())} active, FD spread {spread:.3e}, |GPU - FD| {err:.3e}, |dw| {top:.3g} "
              f"(seeded column {np.max(np.abs(s['dw'][b, :, 0])):.3g})")
        assert spread <= 1e-3 * max(1.0, top), (name, b, "the yardstick itself is too wide")
        assert err <= 4.0 * spread + 1e-6, (name, b)
        seeded = max(seeded, float(np.max(np.abs(s["dw"][b, :, 0]))))
    assert seeded > 1e-3, (name, "the seeded direction must move the solution")


# ------------------------------------------------------------------------------------------
# 5. exact properties
# ------------------------------------------------------------------------------------------
def exact_properties(solver, P, r, seed, alone=None):
    """Zero directions / cotangents give exact zeros; column c of an (nx + 1)-column call (two launches) = that
    column alone; an instance alone = inside its batch (the instances `alone`, default all); a stage-uniform
    direction passed per stage gives the bits of the shared row; the X_0 rows of dw are exact zeros."""
    ocp = solver.ocp
    lin = ocp.model == "linear"
    B, n_w = r["w"].shape
    nx, nu, N = ocp.nx, ocp.nu, ocp.N
    nz = nx + nu
    n_wt = nz * (nz + 1) // 2 if lin else nz
    rng = np.random.default_rng(seed)
    m = nx + 1
    d, g = rng.normal(size=(B, m, n_wt)), rng.normal(size=(B, m, n_w))
    fwd = (lambda d_, P_=P, r_=r: solver.sens_weights(P_, r_, dW=d_)) if lin else \
        (lambda d_, P_=P, r_=r: solver.sens_weights(P_, r_, dQ=d_[..., :nx], dR=d_[..., nx:]))
    keys = ("gWk", "gW") if lin else ("gQk", "gRk", "gQ", "gR")
    s, v = fwd(d), solver.sens_weights_vjp(P, r, g)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    assert s["dw"].shape == (B, n_w, m) and not s["dw"][:, :nx].any()
    assert all(np.all(np.isfinite(v[k])) for k in keys)
    assert np.all(fwd(np.zeros((B, 2, n_wt)))["dw"] == 0.0)
    vz = solver.sens_weights_vjp(P, r, np.zeros((B, 2, n_w)))
    assert all(np.all(vz[k] == 0.0) for k in keys)
    per_stage = np.ascontiguousarray(np.broadcast_to(d[:, :, None, :], (B, m, N, n_wt)))
    assert bits(fwd(per_stage)["dw"]) == bits(s["dw"])
    first = fwd(d[:, :nx]), solver.sens_weights_vjp(P, r, g[:, :nx])
    assert bits(first[0]["dw"]) == bits(s["dw"][:, :, :nx])
    assert all(bits(first[1][k]) == bits(v[k][:, :nx]) for k in keys)
    for c in range(m):
        one = fwd(d[:, c])  # (B, n_wt): a single direction
        assert one["dw"].shape == (B, n_w, 1) and bits(one["dw"][:, :, 0]) == bits(s["dw"][:, :, c]), c
        one = solver.sens_weights_vjp(P, r, g[:, c])
        assert all(bits(one[k][:, 0]) == bits(v[k][:, c]) for k in keys), c
    for b in range(B) if alone is None else alone:
        pt = point_of(r, slice(b, b + 1))
        solo = fwd(d[b:b + 1, :nx], P[b:b + 1], pt)
        assert bits(solo["dw"][0]) == bits(first[0]["dw"][b]) and solo["flag"][0] == 0, b
        solo = solver.sens_weights_vjp(P[b:b + 1], pt, g[b:b + 1, :nx])
        assert all(bits(solo[k][0]) == bits(first[1][k][b]) for k in keys), b
    return s, v


@pytest.mark.parametrize("cost", ["quadrature", "node"])
def test_exact_properties_unicycle(mpcx, cost):
    """5. Unicycle N = 10 with the RK4-quadrature cost (B = 5: the last wave has surplus lanes) and with the node
    cost (the tracking problem), whose gQk of stage 0 is an exact zero (X~_0 = 0)."""
    if cost == "quadrature":
        ocp, P, opts = mpcx.unicycle_point_to_point(N=10), unicycle_P(5, 1), REF_OPTS
    else:
        ocp, P, opts = nonlinear_p_problem("unicycle_tracking_N10")
    solver = mpcx.nlpsol("exact_wt_" + cost, "mi355x", ocp, {"ipopt": opts})
    r = solver.solve_batch(P)
    assert np.all(r["status"] <= 1)
    s, v = exact_properties(solver, P, r, 41)
    assert np.max(np.abs(s["dw"])) > 1e-3 and np.max(np.abs(v["gQk"])) > 1e-3 and np.max(np.abs(v["gRk"])) > 1e-3
    if cost == "node":
        assert not v["gQk"][:, :, 0].any()
    with pytest.raises(ValueError):
        solver.sens_weights(P, r, dQ=np.zeros((P.shape[0] + 1, 3)))
    with pytest.raises(ValueError):
        solver.sens_weights(P, r)
    with pytest.raises(ValueError):
        solver.sens_weights(P, r, dW=np.zeros((P.shape[0], 15)))
    with pytest.raises(ValueError):
        solver.sens_weights_vjp(P, r, np.zeros((P.shape[0], 3, 52)))


@pytest.mark.parametrize("name", ["padded_dint_N8", "ltv_N40"])
def test_exact_properties_linear(mpcx, name):
    lin, P, r, solver, _, _, _, _ = linear_weights_case(name)
    # (a schedule per instance, ltv_N40: a batch of one reads the first row, so instance 0 is the one alone)
    exact_properties(solver, P, r, 42, alone=None if lin.tab.ndim == 1 else [0])


# ------------------------------------------------------------------------------------------
# 6. set_weights
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unicycle_N10", "kin_bicycle_N10"])
def test_set_weights_equals_a_new_handle(mpcx, name):
    """6. A solve (and the sensitivity launches) after set_weights(Q', R') equals, bit for bit, the same on a
    solver created with (Q', R'); a refused call (NaN, a negative entry) leaves the weights as they were."""
    ocp, P, opts = nonlinear_problem(name)
    nx, nu = ocp.nx, ocp.nu
    Q2 = tuple(1.7 * np.array(ocp.Q, float)[:nx] + 0.05)
    R2 = tuple(0.6 * np.array(ocp.R, float)[:nu] + 0.01)
    a = mpcx.nlpsol(name + "_sw_a", "mi355x", ocp, {"ipopt": opts})
    b = mpcx.nlpsol(name + "_sw_b", "mi355x", dataclasses.replace(ocp, Q=Q2, R=R2), {"ipopt": opts})
    before = a.solve_batch(P)
    a.set_weights(Q2, R2)
    assert tuple(a.ocp.Q) == Q2 and tuple(a.ocp.R) == R2
    for bad in ((float("nan"),) + Q2[1:], (-1e-3,) + Q2[1:], (float("inf"),) + Q2[1:]):
        with pytest.raises(mpcx._lib.MpcxError, match="finite and >= 0"):
            a.set_weights(bad, R2)
    with pytest.raises(mpcx._lib.MpcxError, match="finite and >= 0"):
        a.set_weights(Q2, (-1.0,) + R2[1:])
    assert tuple(a.ocp.Q) == Q2 and tuple(a.ocp.R) == R2
    ra, rb = a.solve_batch(P), b.solve_batch(P)
    assert np.all(rb["status"] <= 1)
    for k in ("w", "lam_g", "lam_x", "f", "iters", "status"):
        assert bits(ra[k]) == bits(rb[k]), k
    assert bits(ra["w"]) != bits(before["w"])
    g = np.random.default_rng(7).normal(size=(P.shape[0], 2, ra["w"].shape[1]))
    dQ = np.random.default_rng(8).normal(size=(P.shape[0], 2, nx))
    assert bits(a.sens_weights(P, ra, dQ=dQ)["dw"]) == bits(b.sens_weights(P, rb, dQ=dQ)["dw"])
    va, vb = a.sens_weights_vjp(P, ra, g), b.sens_weights_vjp(P, rb, g)
    assert all(bits(va[k]) == bits(vb[k]) for k in ("gQ", "gR", "gQk", "gRk"))
    with pytest.raises(ValueError):
        a.set_weights(Q2[:-1], R2)


def test_set_weights_refuses_a_linear_model(mpcx):
    lin, P, r, solver, *_ = linear_weights_case("lin4x2_N12")
    with pytest.raises(ValueError):
        solver.set_weights(np.ones(lin.nx), np.ones(lin.nu))
    lib = mpcx._lib.load()
    q, rr = np.ones(lin.nx), np.ones(lin.nu)
    assert lib.mpcx_set_weights(solver._h.ptr, mpcx._lib.dptr(q), mpcx._lib.dptr(rr)) == -1
    assert "tables" in lib.mpcx_last_error().decode()
    assert bits(solver.solve_batch(P)["w"]) == bits(r["w"])
    n = ctypes.c_int32()
    assert lib.mpcx_weight_dims(solver._h.ptr, ctypes.byref(n)) == 0 and n.value == 21  # LinearModel<4,2>: nz = 6


# ------------------------------------------------------------------------------------------
# 7. the device loop
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unicycle_N10", "padded_dint_N8"])
def test_device_loop_equals_host_call(mpcx, name):
    """DeviceLoop.sens_weights / sens_weights_vjp after solve() against the host calls on the loop's tensors copied
    back, bit for bit; every entry of the outputs is written (pre-filled with 7); the point= override on a
    saved copy gives the same bits after the loop has moved on."""
    import torch
    from mpcx.device import DeviceLoop

    if name == "unicycle_N10":
        ocp, P = mpcx.unicycle_point_to_point(N=10), unicycle_P(5, 1)
        solver = mpcx.nlpsol(name + "_wl", "mi355x", ocp, {"ipopt": REF_OPTS})
    else:
        ocp, P = linear_problem(name)
        solver = mpcx.nlpsol(name + "_wl", "mi355x", ocp, {"ipopt": {"max_iter": 300}})
    lin = ocp.model == "linear"
    pd = solver._pad
    B, m, N, nz = P.shape[0], ocp.nx, ocp.N, ocp.nx + ocp.nu
    n_w = 53 if not lin else ocp.n_w_ms
    n_wt_user = nz * (nz + 1) // 2 if lin else nz
    rng = np.random.default_rng(43)
    d, g = rng.normal(size=(B, m, N, n_wt_user)), rng.normal(size=(B, m, n_w))
    loop = DeviceLoop(solver, P, device="cuda:0")
    n_wt = solver._h.weight_dims()
    dk, gk_in = d, g
    if pd is not None:  # the kernel's padded layout
        sel, n_k = solver._wt_sel()
        assert n_k == n_wt
        dk = np.zeros((B, m, N, n_wt))
        dk[..., sel] = d
        gk_in = pd.scatter(g.reshape(B * m, -1), pd.w_idx, pd.n_w_pad).reshape(B, m, -1)
    assert n_wt == (dk.shape[3])
    d_d, d_g = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (dk, gk_in))
    loop.solve()
    nwk = loop.w.shape[1]
    gk_out = torch.full((B, m, N, n_wt), 7.0, dtype=torch.float64, device="cuda:0")
    gs_out = torch.full((B, m, n_wt), 7.0, dtype=torch.float64, device="cuda:0")
    dw_out = torch.full((B, nwk, m), 7.0, dtype=torch.float64, device="cuda:0")
    dw, flag = loop.sens_weights(d_d, dw_out=dw_out)
    gk, gs, vflag = loop.sens_weights_vjp(d_g, gWk_out=gk_out, gW_out=gs_out)
    none_k, gs_only, _ = loop.sens_weights_vjp(d_g, per_stage=False)
    uni = loop.sens_weights(d_d[:, :, 0].contiguous())[0], loop.sens_weights(d_d[:, :, :1].expand(B, m, N, n_wt).contiguous())[0]
    saved = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    torch.cuda.synchronize()
    assert dw is dw_out and gk is gk_out and gs is gs_out and none_k is None
    assert not bool((dw == 7.0).any()) and not bool((gk == 7.0).any()) and not bool((gs == 7.0).any())
    assert bits(gs_only.cpu().numpy()) == bits(gs.cpu().numpy())
    assert bits(uni[0].cpu().numpy()) == bits(uni[1].cpu().numpy())
    host = {k_: t.cpu().numpy() for k_, t in (("P", loop.P), ("w", loop.w), ("lam_g", loop.lam), ("lam_x", loop.lamx))}
    dw_np, gk_np, gs_np = dw.cpu().numpy(), gk.cpu().numpy(), gs.cpu().numpy()
    if pd is not None:
        host = {"P": host["P"][:, pd.p_idx], "w": host["w"][:, pd.w_idx], "lam_g": host["lam_g"][:, pd.g_idx],
                "lam_x": host["lam_x"][:, pd.w_idx]}
        dw_np, gk_np = dw_np[:, pd.w_idx], gk_np[..., sel]
    if lin:
        s, v = solver.sens_weights(host["P"], host, dW=d), solver.sens_weights_vjp(host["P"], host, g)
        assert bits(gk_np) == bits(v["gWk"])
    else:
        s = solver.sens_weights(host["P"], host, dQ=d[..., :ocp.nx], dR=d[..., ocp.nx:])
        v = solver.sens_weights_vjp(host["P"], host, g)
        assert bits(gk_np) == bits(np.concatenate([v["gQk"], v["gRk"]], axis=3))
        assert bits(gs_np) == bits(np.concatenate([v["gQ"], v["gR"]], axis=2))
    assert np.all(s["flag"] == 0) and bits(flag.cpu().numpy()) == bits(s["flag"]) == bits(vflag.cpu().numpy())
    assert bits(dw_np) == bits(s["dw"])
    loop.step()  # the resident point moves on
    loop.solve()
    again = loop.sens_weights(d_d, point=saved)[0], loop.sens_weights_vjp(d_g, point=saved)[0]
    moved = loop.sens_weights(d_d)[0]
    torch.cuda.synchronize()
    assert bits(again[0].cpu().numpy()) == bits(dw.cpu().numpy()) and bits(again[1].cpu().numpy()) == bits(gk.cpu().numpy())
    assert bits(moved.cpu().numpy()) != bits(dw.cpu().numpy())
    with pytest.raises(ValueError):
        loop.sens_weights_vjp(d_g, gW_out=gs_out[:, :1])
    with pytest.raises(ValueError):
        loop.sens_weights(torch.zeros((B, loop._knx + 1, n_wt), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        loop.sens_weights(d_d[..., :-1].contiguous())


# ------------------------------------------------------------------------------------------
# 8. irregular instances: ordinary statuses, nothing faults
# ------------------------------------------------------------------------------------------
def assert_only_irregular(s, v, bad, regular=None):
    for b in range(s["flag"].shape[0]):
        if b == bad:
            assert s["flag"][b] == 1 and v["flag"][b] == 1
            assert np.all(np.isnan(s["dw"][b])) and np.all(np.isnan(v["gWk"][b])) and np.all(np.isnan(v["gW"][b]))
        else:
            assert s["flag"][b] == 0 and v["flag"][b] == 0
            assert np.all(np.isfinite(s["dw"][b])) and np.all(np.isfinite(v["gWk"][b])) and np.all(np.isfinite(v["gW"][b]))
            if regular is not None:  # the neighbours keep their bits
                assert bits(s["dw"][b]) == bits(regular[0]["dw"][b]), b
                assert bits(v["gWk"][b]) == bits(regular[1]["gWk"][b]), b


def test_variable_on_its_bound_is_flagged(mpcx):
    lin, P, r, solver, dW, s, g, v = linear_weights_case("padded_dint_N8")
    w = r["w"].copy()
    w[2, lin.nx + (lin.nx + lin.nu) * 3] = 1.0  # U_3 of instance 2 placed on its upper bound
    pt = {"w": w, "lam_g": r["lam_g"], "lam_x": r["lam_x"]}
    assert_only_irregular(solver.sens_weights(P, pt, dW=dW), solver.sens_weights_vjp(P, pt, g), 2, (s, v))


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
    solver = mpcx.nlpsol("indef_wt", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    P = lin.params(rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    point = {"w": np.zeros((B, lin.n_w_ms)), "lam_g": np.zeros((B, lin.n_g_ms)), "lam_x": np.zeros((B, lin.n_w_ms))}
    d, g = rng.normal(size=(B, 2, 15)), rng.normal(size=(B, 2, lin.n_w_ms))
    assert_only_irregular(solver.sens_weights(P, point, dW=d), solver.sens_weights_vjp(P, point, g), 1)


# ------------------------------------------------------------------------------------------
# 9. refusals: MPCX_EINVAL with a message, nothing launched
# ------------------------------------------------------------------------------------------
def test_refusals(mpcx):
    """m = 0 and m = nx + 1, N = 64, null pointers, B < 1, a null handle, on all four entry points; both
    outputs of the reverse mode null."""
    import torch
    from mpcx import _lib

    lib = _lib.load()
    EINVAL = -1

    def host_call(solver, vjp, B=2, m=1, n_null=()):
        h = solver._h
        n, mm, N = max(B, 1), max(m, 1), solver.ocp.N
        arr = [np.zeros((n, h.n_p)), np.zeros((n, h.n_w)), np.zeros((n, h.n_g)), np.zeros((n, h.n_w)),
               np.zeros((n, mm, max(h.n_w, N * 5))), np.full((n, mm, N, 5), 7.0), np.full((n, h.n_w, mm), 7.0)]
        a = [None if i in n_null else _lib.dptr(x) for i, x in enumerate(arr)]
        if vjp:  # gw = arr[4]; gWk = arr[5]; gW = arr[6] (larger than needed)
            rc = lib.mpcx_sens_weights_vjp(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], m, a[5], a[6], None)
        else:  # dW = arr[4] (per stage); dw = arr[6]
            rc = lib.mpcx_sens_weights(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], 1, m, a[6], None)
        assert rc != 0 and np.all(arr[5] == 7.0) and np.all(arr[6] == 7.0)
        return rc, lib.mpcx_last_error().decode()

    solver = mpcx.nlpsol("ok_wt", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    long = mpcx.nlpsol("n64_wt", "mi355x", mpcx.unicycle_point_to_point(N=64), {"ipopt": REF_OPTS})
    buf = torch.zeros(2 * long._h.n_w * 4, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())

    def dev_call(h, vjp, B=2, m=1, lam_g=p, a=p, b=p, c=p):
        if vjp:
            rc = lib.mpcx_sens_weights_vjp_dev(h.ptr if h else None, B, p, p, lam_g, p, a, m, b, c, None, None)
        else:
            rc = lib.mpcx_sens_weights_dev(h.ptr if h else None, B, p, p, lam_g, p, a, 1, m, b, None, None)
        return rc, lib.mpcx_last_error().decode()

    for vjp in (False, True):
        who = "sens_weights_vjp" if vjp else "sens_weights:"
        for call, ok, n64 in ((host_call, solver, long), (dev_call, solver._h, long._h)):
            for m in (0, 4):
                rc, msg = call(ok, vjp, m=m)
                assert rc == EINVAL and "between 1 and nx" in msg and who in msg, (m, msg)
            for B in (0, -3):
                rc, msg = call(ok, vjp, B=B)
                assert rc == EINVAL and "B must be >= 1" in msg
            rc, msg = call(n64, vjp)
            assert rc == EINVAL and "N >= 64" in msg
        for i in (0, 1, 2, 3, 4) + (() if vjp else (6,)):  # P, w, lam_g, lam_x, the directions / cotangents, dw
            rc, msg = host_call(solver, vjp, n_null=(i,))
            assert rc == EINVAL and "required" in msg, i
        if vjp:  # one of the two outputs is enough, none is refused
            rc, msg = host_call(solver, True, n_null=(5, 6))
            assert rc == EINVAL and "required" in msg
            rc, msg = dev_call(solver._h, True, b=None, c=None)
            assert rc == EINVAL and "required" in msg
        for kw in ({"lam_g": None}, {"a": None}) + (() if vjp else ({"b": None},)):
            rc, msg = dev_call(solver._h, vjp, **kw)
            assert rc == EINVAL and "required" in msg, kw
        rc, msg = dev_call(None, vjp)
        assert rc == EINVAL and "null handle" in msg
    assert lib.mpcx_weight_dims(None, None) == EINVAL and lib.mpcx_set_weights(None, None, None) == EINVAL
    n = ctypes.c_int32()
    assert lib.mpcx_weight_dims(solver._h.ptr, ctypes.byref(n)) == 0 and n.value == 5
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched


# ------------------------------------------------------------------------------------------
# 10. autograd
# ------------------------------------------------------------------------------------------
def fd_of_loss(solver, P, nom, Q, R, loss, idx):
    """{h: central differences of loss(w) in the weights idx (positions in (Q, R)) through set_weights}, h = 1e-3
    and 1e-4 relative to each weight, warm-started from the nominal solution; the weights are put back."""
    nx = len(Q)
    wt = np.concatenate([Q, R])
    out = {}
    for h in (1e-3, 1e-4):
        row = []
        for i in idx:
            val = []
            for sgn in (1.0, -1.0):
                moved = wt.copy()
                moved[i] += sgn * h * wt[i]
                solver.set_weights(moved[:nx], moved[nx:])
                r = solver.solve_batch(P, w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"])
                assert np.all(r["status"] <= 1)
                val.append(loss(r["w"]))
            row.append((val[0] - val[1]) / (2 * h * wt[i]))
        out[h] = np.array(row)
    solver.set_weights(Q, R)
    return out


@pytest.mark.parametrize("name", ["unicycle_N10", "path_bicycle_N20"])
def test_autograd_weights(mpcx, name):
    """10. solve_differentiable(loop, P, Q=, R=): Q.grad, R.grad of an imitation loss on U_0 against central
    differences of the loss through set_weights (h = 1e-3 and 1e-4 relative to each weight, solver at tol =
    1e-10; tolerance 4 x spread + 1e-6 against the mean, spread <= 1e-3 max(1, |gradient|_max); a weight that
    is zero cannot be moved both ways and is left to the identity tests).  The unicycle (B = 4) with P requiring
    a gradient too; the path-frame bicycle, which has no sens_vjp, with weight gradients alone.  The backward
    differentiates at the forward's weights also after another solve has changed the solver's, and puts the
    changed ones back.  Measured on one MI355X (spread, |autograd - FD|): unicycle_N10 1.8e-6, 8.9e-7;
    path_bicycle_N20 3.8e-5, 2.0e-5 on a gradient of 47."""
    import torch
    from mpcx.autograd import MPCWeightsFunction, solve_differentiable
    from mpcx.device import DeviceLoop

    ocp, P0, opts = nonlinear_problem(name)
    solver = mpcx.nlpsol(name + "_ag_w", "mi355x", ocp, {"ipopt": dict(opts, tol=1e-10)})
    B, nx, nu = P0.shape[0], ocp.nx, ocp.nu
    Q0, R0 = np.array(ocp.Q, float)[:nx], np.array(ocp.R, float)[:nu]
    with_P = name == "unicycle_N10"
    t64 = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device="cuda:0", requires_grad=grad)  # noqa: E731
    u_np = np.random.default_rng(19).uniform(-0.5, 0.5, (B, nu))
    u_t = t64(u_np)
    loss_np = lambda w: 0.5 * float(np.sum((w[:, nx:nx + nu] - u_np) ** 2))  # noqa: E731
    grads = []
    for change in (False, True):
        loop = DeviceLoop(solver, P0, device="cuda:0")
        P, Q, R = t64(P0, with_P), t64(Q0, True), t64(R0, True)
        w = solve_differentiable(loop, P, Q=Q, R=R)
        assert w.shape == (B, loop.w.shape[1]) and type(w.grad_fn).__name__ == MPCWeightsFunction.__name__ + "Backward"
        point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
        gw = torch.zeros((B, 1, w.shape[1]), dtype=torch.float64, device="cuda:0")
        gw[:, 0, nx:nx + nu] = (w[:, nx:nx + nu] - u_t).detach()
        _, direct, flag = loop.sens_weights_vjp(gw, point=point, per_stage=False)
        gP = loop.sens_vjp(gw, point=point)[0] if with_P else None
        other = (tuple(2.0 * Q0 + 0.1), tuple(0.5 * R0 + 0.1))
        if change:  # another solve with other weights after the forward: the backward must not use them
            solver.set_weights(*other)
            loop.solve()
        (0.5 * ((w[:, nx:nx + nu] - u_t) ** 2).sum()).backward()
        torch.cuda.synchronize()
        assert int(flag.sum()) == 0
        if change:
            assert (tuple(solver.ocp.Q), tuple(solver.ocp.R)) == other
        tot = direct[:, 0].sum(dim=0).cpu().numpy()
        assert bits(Q.grad.cpu().numpy()) == bits(tot[:nx]) and bits(R.grad.cpu().numpy()) == bits(tot[nx:])
        if with_P:
            assert bits(P.grad.cpu().numpy()) == bits(gP[:, 0].cpu().numpy())
        else:
            assert P.grad is None
        grads.append(np.concatenate([Q.grad.cpu().numpy(), R.grad.cpu().numpy()]))
        solver.set_weights(Q0, R0)
    assert bits(grads[0]) == bits(grads[1])
    grad = grads[0]
    nom = solver.solve_batch(P0)
    idx = np.flatnonzero(np.concatenate([Q0, R0]) > 0)
    fd = fd_of_loss(solver, P0, nom, Q0, R0, loss_np, idx)
    spread = float(np.max(np.abs(fd[1e-3] - fd[1e-4])))
    err = float(np.max(np.abs(grad[idx] - 0.5 * (fd[1e-3] + fd[1e-4]))))
    print(f"{name}: gradient {grad}, FD spread {spread:.3e}, |autograd - FD| {err:.3e}")
    assert spread <= 1e-3 * max(1.0, float(np.max(np.abs(grad))))
    assert err <= 4.0 * spread + 1e-6
    assert np.max(np.abs(grad)) > 1e-3
    # irregular="zero" is accepted as before; the excluded combinations raise
    loop = DeviceLoop(solver, P0, device="cuda:0")
    Q, R = t64(Q0, True), t64(R0, True)
    solve_differentiable(loop, t64(P0), irregular="zero", Q=Q, R=R).sum().backward()
    assert bool(torch.isfinite(Q.grad).all())
    lbw = t64(np.zeros((B, loop.w.shape[1])))
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), Q=Q, R=R, lbw=lbw, ubw=lbw + 1.0)
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), Q=Q)
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), Q=Q[:-1], R=R)
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), Q=Q.to(torch.float32), R=R)


def test_autograd_weights_refuses_a_linear_model(mpcx):
    import torch
    from mpcx.autograd import solve_differentiable
    from mpcx.device import DeviceLoop

    lin, P = linear_problem("lin4x2_N12")
    solver = mpcx.nlpsol("ag_w_lin", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    loop = DeviceLoop(solver, P, device="cuda:0")
    Q, R = (torch.ones(n, dtype=torch.float64, device="cuda:0", requires_grad=True) for n in (lin.nx, lin.nu))
    with pytest.raises(ValueError, match="tables"):
        solve_differentiable(loop, loop.P.clone(), Q=Q, R=R)
