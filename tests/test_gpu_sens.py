"""GPU tests of the sensitivities of the MPC solution to the initial state (mpcx_sens_x0 /
mpcx_sens_x0_dev, Solver.sens_x0, DeviceLoop.sens_x0; csrc/sens.h).

References: tests/helpers/sens_ref.py -- (a) the kernel's recursion restated in long double from the
GPU's own point, (b) the active-set sensitivities -- and, for the nonlinear models, central
differences of the solver itself.  Shapes are the smallest that reach every lane group (16, 32, 64)
and every solve unit."""
import ctypes
import dataclasses
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sens_ref as sr  # noqa: E402

REF_OPTS = {"max_iter": 2000, "acceptable_tol": 1e-8, "acceptable_obj_change_tol": 1e-6}
LD = np.longdouble


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


# ------------------------------------------------------------------------------------------
# linear cases (tests 1 and 2): solved once, shared, never modified
# ------------------------------------------------------------------------------------------
LINEAR_CASES = ("padded_dint_N8", "lin4x2_N12", "cartpole_qp_N50", "ltv_N40")


def linear_problem(name):
    from mpcx import lti

    if name == "padded_dint_N8":  # LinearModel<4,1> with two pad states, G = 16; x0 = 5 saturates the input
        N, T = 8, 0.1
        A, Bm = np.array([[1.0, T], [0.0, 1.0]]), np.array([[0.5 * T * T], [T]])
        lin = lti.LinearOCP(N=N, A=A[None], B=Bm[None], W=np.diag([1.0, 0.1, 0.01])[None],
                            tab=np.zeros(N, np.int32), u_lb=(-1.0,), u_ub=(1.0,))
        # (x0 = 5 saturates the input for 7 of the 8 moves; the others: strictly complementary solutions too)
        x0 = np.array([[5.0, 0.0], [2.0, 2.0], [-1.0, 0.0], [-6.0, 0.5], [-0.2, 0.1]])
        return lin, lin.params(x0, np.zeros((N, 3)))
    if name == "lin4x2_N12":  # LinearModel<4,2>, random stable tables, G = 16; 4 to 10 active input bounds each
        rng = np.random.default_rng(5)
        nx, nu, N = 4, 2, 12
        A = rng.normal(size=(nx, nx))
        A *= 0.95 / np.max(np.abs(np.linalg.eigvals(A)))
        Bm = rng.normal(size=(nx, nu))
        lin = lti.LinearOCP(N=N, A=A[None], B=Bm[None], W=np.diag([1.0, 2.0, 1.0, 0.5, 0.1, 0.2])[None],
                            tab=np.zeros(N, np.int32), u_lb=(-0.5, -0.5), u_ub=(0.5, 0.5))
        x0 = 3.0 * rng.normal(size=(24, nx))[[0, 1, 2, 4]]  # (draw 3 ends with a weakly active input)
        return lin, lin.params(x0, np.zeros((N, nx + nu)))
    if name == "cartpole_qp_N50":  # LinearModel<5,1>: sequential chain with the decoupled suffix, G = 64
        lin = lti.inverted_pendulum_qp(N=50)
        x = np.array([[0.0, 0.0, 0.1, 0.0], [9.0, 0.5, -0.1, 0.2]])
        return lin, lti.pendulum_params(lin, x, 0.0)
    assert name == "ltv_N40"  # LinearModel<4,1>, per-instance tables, G = 64; instance 0 has an active steering bound
    pick = [0, 9]
    lin = lti.lateral_ltv(N=40, Delta=0.05, vref=[8.0, 12.0], delta_max=0.02, per_instance_tab=np.arange(24)[pick] % 2)
    x0 = np.random.default_rng(2).normal(size=(24, 4))[pick] * np.array([0.5, 0.05, 0.2, 0.05])
    return lin, lin.params(x0, np.zeros((40, 5)))


@functools.lru_cache(maxsize=None)
def linear_case(name):
    """(lin, P, solve result, sens result, solver) of a linear case"""
    import mpcx

    lin, P = linear_problem(name)
    solver = mpcx.nlpsol(name, "mi355x", lin, {"ipopt": {"max_iter": 300}})
    r = solver.solve_batch(P)
    assert np.all(r["status"] == 0), (name, r["status"])
    s = solver.sens_x0(P, r)
    for v in (*r.values(), *s.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lin, P, r, s, solver


def restated(lin, r, b, dtype):
    """helper (a) fed the GPU's point of instance b and the tables"""
    lb, ub = sr.ocp_bounds(lin)
    A, Bm, H = sr.linear_operands(lin, b)
    Sig = sr.sigma_of(r["w"][b], r["lam_x"][b], lb, ub, lin.nx, lin.nu, dtype)
    return sr.riccati_sens(A, Bm, H, Sig, dtype)


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_restatement(mpcx, name):
    """1. The kernel against its recursion restated in long double at the same point (w, lam_x) and
    tables: 64 x E_ref relative to max(1, |entry|), the convention of tests/test_gpu_scan.py::scan_tolerance
    (E_ref = the float64 restatement's own worst error against long double, 6.1e-16, so 3.9e-14).
    Measured on one MI355X: padded_dint_N8 1.5e-16, lin4x2_N12 6.1e-17, ltv_N40 9.9e-17,
    cartpole_qp_N50 1.5e-15.  The last one is what the kernel's refinement step is for: its 45
    move-blocked stages run P_k = Q + A^T P_{k+1} A over an unstable open loop, and the two sweeps
    alone gave 1.06e-13 there (the float64 NumPy restatement 4.0e-13; tests/test_sens_cpu.py
    test_refinement_on_an_unstable_open_loop restates the step)."""
    lin, P, r, s, _ = linear_case(name)
    tol = 64.0 * sr.e_ref()
    assert np.all(s["flag"] == 0), s["flag"]
    assert s["dw_dx0"].shape == (P.shape[0], lin.n_w_ms, lin.nx) and s["K0"].shape == (P.shape[0], lin.nu, lin.nx)
    worst = 0.0
    for b in range(P.shape[0]):
        ref, ok = restated(lin, r, b, LD)
        assert ok
        worst = max(worst, sr.rel_err(s["dw_dx0"][b], ref))
    print(f"{name}: worst error against the long-double restatement {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_active_set(mpcx, name):
    """2. Against the active-set sensitivities (helper (b): active variables fixed, no barrier term).
    Asserted on the inputs: every bounded variable is active (slack < 1e-6, |lam_x| > 1e-2) or has
    |lam_x| < 1e-7.  Tolerance: 8 x the distance helper (a) in long double, fed the same GPU point,
    has to (b) -- the barrier term's own O(mu) gap; the rows of the active variables are within it
    of zero.  Measured distances of (a) to (b) on one MI355X, worst instance of each case:
    padded_dint_N8 5.4e-5 (the instance without an active bound; 5.2e-8 to 9.8e-7 on the saturated
    ones), lin4x2_N12 1.4e-6, cartpole_qp_N50 3.7e-8, ltv_N40 1.5e-7; the GPU's distance to (b) equals
    (a)'s to three digits in every instance."""
    lin, P, r, s, _ = linear_case(name)
    lb, ub = sr.ocp_bounds(lin)
    n_act = 0
    for b in range(P.shape[0]):
        act, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, lin.nx)
        assert ok, (name, b, "a bounded variable is neither active nor without a multiplier")
        n_act += int(act.sum())
        A, Bm, H = sr.linear_operands(lin, b)
        ref = sr.active_set_sens(A, Bm, H, act)
        dist = float(np.max(np.abs(np.asarray(restated(lin, r, b, LD)[0], np.float64) - ref)))
        err = float(np.max(np.abs(s["dw_dx0"][b] - ref)))
        print(f"{name} b={b}: {int(act.sum())} active, (a)-(b) {dist:.3e}, GPU-(b) {err:.3e}")
        assert err <= 8.0 * dist
        if act.any():
            assert np.max(np.abs(s["dw_dx0"][b][act])) <= 8.0 * dist
    assert n_act > 0 or name == "cartpole_qp_N50", "the case must have active bounds"  # (|u| <= 200 is never reached)


# ------------------------------------------------------------------------------------------
# 3. nonlinear models against central differences of the solver itself
# ------------------------------------------------------------------------------------------
NONLINEAR_CASES = ("unicycle_N10", "unicycle_bounded_N10", "unicycle_N30", "kin_bicycle_N10", "cartpole_N20",
                   "path_bicycle_N20", "dyn_bicycle_N10")


def unicycle_P(B, seed):
    rng = np.random.default_rng(seed)
    P = np.zeros((B, 6))
    P[:, 0:2] = rng.uniform(-0.3, 0.3, (B, 2))
    P[:, 2] = rng.uniform(-0.5, 0.5, B)
    P[:, 3] = rng.uniform(1.0, 2.0, B)
    P[:, 4] = rng.uniform(0.5, 1.5, B)
    P[:, 5] = rng.uniform(-0.3, 0.3, B)
    return P


def nonlinear_problem(name):
    """(ocp, P, ipopt options)"""
    import mpcx
    from mpcx import ode

    # (the draws picked are those whose solutions are strictly complementary: 6 to 18 active input bounds each)
    if name == "unicycle_N10":  # the x-free unit, G = 16
        return mpcx.unicycle_point_to_point(N=10), unicycle_P(24, 1)[[0, 5, 6, 7]], REF_OPTS
    if name == "unicycle_bounded_N10":  # a finite state bound (y <= 1, active at the last node of instance 3): the bounded unit
        ocp = dataclasses.replace(mpcx.unicycle_point_to_point(N=10), x_ub=(math.inf, 1.0, math.inf))
        return ocp, unicycle_P(24, 1)[[0, 5, 6, 12]], REF_OPTS
    if name == "unicycle_N30":  # the scan unit, G = 32
        return mpcx.unicycle_point_to_point(N=30), unicycle_P(24, 1)[[1, 7, 8, 9]], REF_OPTS
    if name == "kin_bicycle_N10":
        B, N = 4, 10
        rng = np.random.default_rng(2)
        ocp = ode.kinematic_bicycle_tracking(N=N)
        ref = ode.bicycle_circular_reference(rng.uniform(0, 20 * math.pi, B), 0, N)
        return ocp, ocp.params(ref[:, 0, :3] + rng.normal(0, 0.1, (B, 3)), ref), {"max_iter": 500}
    if name == "cartpole_N20":
        B = 4
        rng = np.random.default_rng(3)
        ocp = ode.cartpole_swingup(N=20)
        x0 = rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.3])
        xr = np.zeros((B, 4))
        xr[:, 0] = rng.uniform(-1, 1, B)
        return ocp, ocp.params(x0, xr), {"max_iter": 1000}
    if name == "dyn_bicycle_N10":  # the 6-state bicycle: its chain written out in the kernel (no workspace stash)
        B, N = 3, 10
        rng = np.random.default_rng(4)
        ocp = ode.dynamic_bicycle_lane_change(N=N)
        ref = np.zeros((B, N, 8))
        ref[..., 0] = 6.0 * ocp.T * np.arange(N)
        ref[..., 3] = 6.0
        x0 = ref[:, 0, :6] + rng.normal(0, 1, (B, 6)) * np.array([0.2, 0.2, 0.05, 0.3, 0.1, 0.05])
        return ocp, ocp.params(x0, ref), {"max_iter": 1000}
    assert name == "path_bicycle_N20"
    B, N, pick = 24, 20, [0, 1, 3, 4]
    rng = np.random.default_rng(6)
    ocp = ode.path_bicycle_lane_keeping(N=N)
    rows = np.zeros((B, N, 6))
    rows[..., 0] = rng.uniform(-0.5, 0.5, (B, 1))
    rows[..., 2] = rng.uniform(5.0, 10.0, (B, 1))
    x = np.stack([rows[:, 0, 0] + rng.uniform(-0.3, 0.3, B), rng.normal(0, 0.02, B),
                  rows[:, 0, 2] + rng.normal(0, 0.3, B)], axis=1)
    return ocp, ode.path_bicycle_params(ocp, x[pick], 0.0, rows[pick]), {"max_iter": 1000, "tol": 1e-8}


@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_nonlinear_against_finite_differences(mpcx, name):
    """3. dw*/dx0 against central differences of solve_batch in each component of x0, warm-started
    from the nominal solution, at h = 1e-3 and h = 1e-4.  Yardstick: the spread between the two
    estimates (their largest difference over the instance's entries); tolerance 4 x spread + 1e-6
    against their mean.  An instance whose active set (classes (i) / (ii) of helpers/sens_ref.py
    classify) changes between x0 +- h is left out, at most one per case; the nominal solutions are
    strictly complementary (asserted).  Measured on one MI355X, worst instance of each case (FD
    spread, |GPU - FD|): unicycle_N10 3.4e-5, 5.5e-6; unicycle_bounded_N10 3.1e-5, 5.0e-6;
    unicycle_N30 1.9e-4, 9.3e-5; kin_bicycle_N10 4.8e-5, 2.3e-5; cartpole_N20 2.7e-5, 1.4e-5;
    path_bicycle_N20 1.2e-5, 6.1e-6; dyn_bicycle_N10 1.1e-4, 5.5e-5.  (The spread is the solver's
    own convergence noise, ~1e-8 in w, divided by 2 h = 2e-4.)"""
    ocp, P, opts = nonlinear_problem(name)
    solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": opts})
    nx, B = ocp.nx, P.shape[0]
    lb, ub = sr.ocp_bounds(ocp)
    nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), nom["status"]
    s = solver.sens_x0(P, nom)
    assert np.all(s["flag"] == 0), s["flag"]
    act0 = []
    for b in range(B):
        a, ok = sr.classify(nom["w"][b], nom["lam_x"][b], lb, ub, nx)
        assert ok, (name, b, "the nominal solution is not strictly complementary")
        act0.append(a)
    same = np.ones(B, bool)
    fd = {}
    for h in (1e-3, 1e-4):
        d = np.zeros((B, nom["w"].shape[1], nx))
        for j in range(nx):
            side = []
            for sgn in (1.0, -1.0):
                Pp = P.copy()
                Pp[:, j] += sgn * h
                r = solver.solve_batch(Pp, w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"])
                for b in range(B):
                    a, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, nx)
                    same[b] &= bool(r["status"][b] <= 1 and ok and np.array_equal(a, act0[b]))
                side.append(r["w"])
            d[:, :, j] = (side[0] - side[1]) / (2 * h)
        fd[h] = d
    assert np.count_nonzero(~same) <= 1, (name, "instances whose active set changes", np.flatnonzero(~same))
    for b in np.flatnonzero(same):
        spread = float(np.max(np.abs(fd[1e-3][b] - fd[1e-4][b])))
        err = float(np.max(np.abs(s["dw_dx0"][b] - 0.5 * (fd[1e-3][b] + fd[1e-4][b]))))
        print(f"{name} b={b}: {int(act0[b].sum())} active, FD spread {spread:.3e}, |GPU - FD| {err:.3e}, "
              f"|K0| {np.max(np.abs(s['K0'][b])):.3f}")
        assert err <= 4.0 * spread + 1e-6, (name, b)
        if not act0[b][nx:nx + ocp.nu].any():  # (a saturated U_0 does not move with x0)
            assert np.max(np.abs(s["K0"][b])) > 1e-3  # the feedback gain is kept, not zeroed


# ------------------------------------------------------------------------------------------
# 4. exact properties
# ------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("name", ["padded_dint_N8", "ltv_N40"])
def test_exact_rows_linear(mpcx, name):
    lin, P, r, s, _ = linear_case(name)
    for b in range(P.shape[0]):
        assert bits(s["dw_dx0"][b, :lin.nx]) == bits(np.eye(lin.nx))
        assert bits(s["K0"][b]) == bits(s["dw_dx0"][b, lin.nx:lin.nx + lin.nu])


def test_exact_properties_unicycle(mpcx):
    """dX_0/dx0 = I and K0 = rows nx:nx+nu of dw_dx0, bit for bit; instance b inside B = 5 equals the
    same instance alone; the single-shooting form returns the control rows."""
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("exact", "mi355x", ocp, {"ipopt": REF_OPTS})
    P = unicycle_P(5, 1)
    r = solver.solve_batch(P)
    s = solver.sens_x0(P, r)
    assert np.all(s["flag"] == 0)
    for b in range(5):
        assert bits(s["dw_dx0"][b, :3]) == bits(np.eye(3))
        assert bits(s["K0"][b]) == bits(s["dw_dx0"][b, 3:5])
        solo = solver.sens_x0(P[b:b + 1], {k: r[k][b:b + 1] for k in ("w", "lam_g", "lam_x")})
        for key in ("dw_dx0", "K0", "flag"):
            assert bits(solo[key][0]) == bits(s[key][b]), (b, key)
    ss = mpcx.nlpsol("ss", "mi355x", mpcx.unicycle_point_to_point(N=10, formulation="single_shooting"),
                     {"ipopt": REF_OPTS})
    su = ss.sens_x0(P, r)
    rows = np.concatenate([3 + 5 * k + np.arange(2) for k in range(10)])
    assert su["dw_dx0"].shape == (5, 20, 3) and bits(su["dw_dx0"]) == bits(s["dw_dx0"][:, rows])


@pytest.mark.parametrize("name", ["unicycle_N10", "padded_dint_N8"])
def test_device_loop_equals_host_call(mpcx, name):
    """Host and device entry points give the same bits: DeviceLoop.sens_x0 after solve() and after
    step() (P already advanced: not a solution's own x0, but the same data) against Solver.sens_x0
    on the loop's tensors copied back."""
    import torch
    from mpcx.device import DeviceLoop

    if name == "unicycle_N10":
        ocp, P = mpcx.unicycle_point_to_point(N=10), unicycle_P(5, 1)
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": REF_OPTS})
    else:
        ocp, P = linear_problem(name)
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": {"max_iter": 300}})
    pd = solver._pad
    loop = DeviceLoop(solver, P, device="cuda:0")
    for phase in ("solve", "step"):
        getattr(loop, phase)()
        dw, K0, flag = loop.sens_x0()
        torch.cuda.synchronize()
        host = {k: t.cpu().numpy() for k, t in (("P", loop.P), ("w", loop.w), ("lam_g", loop.lam), ("lam_x", loop.lamx))}
        dw, K0 = dw.cpu().numpy(), K0.cpu().numpy()
        if pd is not None:  # the loop's tensors hold the kernel's padded layout
            host = {"P": host["P"][:, pd.p_idx], "w": host["w"][:, pd.w_idx], "lam_g": host["lam_g"][:, pd.g_idx],
                    "lam_x": host["lam_x"][:, pd.w_idx]}
            dw, K0 = dw[:, pd.w_idx, :ocp.nx], K0[:, :, :ocp.nx]
        s = solver.sens_x0(host["P"], host)
        assert np.all(s["flag"] == 0) and bits(flag.cpu().numpy()) == bits(s["flag"]), phase
        assert bits(dw) == bits(s["dw_dx0"]) and bits(K0) == bits(s["K0"]), phase
    out = torch.full((P.shape[0], solver._h.n_w, loop._knx), 7.0, dtype=torch.float64, device="cuda:0")
    got = loop.sens_x0(dw_out=out)[0]
    torch.cuda.synchronize()
    assert got is out and not bool((out == 7.0).any())
    with pytest.raises(ValueError):
        loop.sens_x0(K0_out=out)


# ------------------------------------------------------------------------------------------
# 5. irregular instances: ordinary statuses, nothing faults
# ------------------------------------------------------------------------------------------
def assert_only_irregular(s, bad):
    B = s["flag"].shape[0]
    for b in range(B):
        if b == bad:
            assert s["flag"][b] == 1
            assert np.all(np.isnan(s["dw_dx0"][b])) and np.all(np.isnan(s["K0"][b]))
        else:
            assert s["flag"][b] == 0
            assert np.all(np.isfinite(s["dw_dx0"][b])) and np.all(np.isfinite(s["K0"][b]))


def test_indefinite_stage_is_flagged(mpcx):
    """A negative input weight on the last stage (x_N carries no cost, so Huu' = 2 W_uu < 0 there), as
    in test_scan_fallback_on_indefinite_stage_weights, on instance 1 of 3 through per-instance tables."""
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
    solver = mpcx.nlpsol("indef", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    P = lin.params(rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    point = {"w": np.zeros((B, lin.n_w_ms)), "lam_g": np.zeros((B, lin.n_g_ms)), "lam_x": np.zeros((B, lin.n_w_ms))}
    assert_only_irregular(solver.sens_x0(P, point), 1)


def test_variable_on_its_bound_is_flagged(mpcx):
    lin, P, r, s, solver = linear_case("padded_dint_N8")
    w = r["w"].copy()
    w[2, lin.nx + (lin.nx + lin.nu) * 3] = 1.0  # U_3 of instance 2 placed on its upper bound
    assert_only_irregular(solver.sens_x0(P, {"w": w, "lam_g": r["lam_g"], "lam_x": r["lam_x"]}), 2)


# ------------------------------------------------------------------------------------------
# 6. refusals: MPCX_EINVAL with a message, nothing launched
# ------------------------------------------------------------------------------------------
def test_refusals(mpcx):
    from mpcx import _lib

    lib = _lib.load()
    EINVAL = -1

    def host_call(solver, B, n_null=(), dw=True, K0=True):
        h = solver._h
        nx, nu = solver.ocp.nx, solver.ocp.nu
        n = max(B, 1)
        arr = [np.zeros((n, h.n_p)), np.zeros((n, h.n_w)), np.zeros((n, h.n_g)), np.zeros((n, h.n_w))]
        args = [None if i in n_null else _lib.dptr(a) for i, a in enumerate(arr)]
        out = np.zeros((n, h.n_w, nx)), np.zeros((n, nu, nx)), np.zeros(n, np.int32)
        rc = lib.mpcx_sens_x0(h.ptr, B, *args, None, None, _lib.dptr(out[0]) if dw else None,
                              _lib.dptr(out[1]) if K0 else None, _lib.iptr(out[2]))
        return rc, lib.mpcx_last_error().decode()

    solver = mpcx.nlpsol("ok", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    for B in (0, -3):
        rc, msg = host_call(solver, B)
        assert rc == EINVAL and "B must be >= 1" in msg
    for i in range(4):
        rc, msg = host_call(solver, 2, n_null=(i,))
        assert rc == EINVAL and "required" in msg
    rc, msg = host_call(solver, 2, dw=False, K0=False)
    assert rc == EINVAL and "at least one" in msg
    assert host_call(solver, 2, dw=False)[0] == 0 and host_call(solver, 2, K0=False)[0] == 0
    long = mpcx.nlpsol("n64", "mi355x", mpcx.unicycle_point_to_point(N=64), {"ipopt": REF_OPTS})
    rc, msg = host_call(long, 2)
    assert rc == EINVAL and "N >= 64" in msg
    # the device entry point refuses the same (real device buffers, large enough for either handle)
    import torch

    buf = torch.zeros(2 * long._h.n_w * 3, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())

    def dev_call(h, B, lam_g=p, dw=p, K0=p):
        rc = lib.mpcx_sens_x0_dev(h.ptr, B, p, p, lam_g, p, dw, K0, None, None)
        return rc, lib.mpcx_last_error().decode()

    rc, msg = dev_call(long._h, 2)
    assert rc == EINVAL and "N >= 64" in msg
    rc, msg = dev_call(solver._h, 2, lam_g=None)
    assert rc == EINVAL and "required" in msg
    rc, msg = dev_call(solver._h, 2, dw=None, K0=None)
    assert rc == EINVAL and "at least one" in msg
    rc, msg = dev_call(solver._h, 0)
    assert rc == EINVAL and "B must be >= 1" in msg
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched
