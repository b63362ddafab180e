"""GPU tests of the directional sensitivities of the MPC solution to the whole parameter row
(mpcx_sens_p / mpcx_sens_p_dev, Solver.sens_p, Solver.sens_xref, DeviceLoop.sens_p; csrc/sens.h
sens_p_kernel).

References: tests/helpers/sens_p_ref.py -- (a) the affine recursion restated in long double from the
GPU's own point, (c) the parametric active-set sensitivities -- and, for the nonlinear models, central
differences of the solver itself along the directions.  Cases and shapes are those of
tests/test_gpu_sens.py (its constructors are imported): the smallest that reach every lane group
(16, 32, 64) and every solve unit."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sens_p_ref as sp  # noqa: E402
import sens_ref as sr  # noqa: E402
from test_gpu_sens import LINEAR_CASES, REF_OPTS, linear_case, linear_problem, nonlinear_problem, unicycle_P  # noqa: E402

LD = np.longdouble


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------------------------------
# linear cases (tests 1 to 3): the solves of test_gpu_sens.py's linear_case, shared, never modified
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_p_case(name):
    """(lin, P, solve result, solver, dP (B, nx, n_p) seeded normal over the whole row, sens_p result)"""
    lin, P, r, _, solver = linear_case(name)
    dP = np.random.default_rng(100 + LINEAR_CASES.index(name)).normal(size=(P.shape[0], lin.nx, P.shape[1]))
    s = solver.sens_p(P, r, dP)
    for v in (dP, *s.values()):
        v.setflags(write=False)
    return lin, P, r, solver, dP, s


def restated_p(lin, r, b, dPb, dtype):
    """helper (a) fed the GPU's point of instance b, the tables and the directions dPb (m, n_p)"""
    lb, ub = sr.ocp_bounds(lin)
    A, Bm, H = sr.linear_operands(lin, b)
    Sig = sr.sigma_of(r["w"][b], r["lam_x"][b], lb, ub, lin.nx, lin.nu, dtype)
    return sp.affine_sens(A, Bm, H, Sig, *sp.linear_rhs(lin, np.asarray(dPb, dtype), b), dtype)


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_restatement(mpcx, name):
    """1. The kernel against the affine recursion restated in long double at the same point and tables,
    m = nx seeded normal directions over the whole of P (x0 part included): 64 x e_ref_p relative to
    max(1, |entry|), the convention of tests/test_gpu_scan.py::scan_tolerance and of test_gpu_sens.py's
    test 1 (e_ref_p = the float64 restatement's own worst error against long double).
    Measured on one MI355X (e_ref_p = 1.9e-15, tolerance 1.2e-13): padded_dint_N8 1.2e-16, lin4x2_N12
    1.2e-16, ltv_N40 1.1e-16, cartpole_qp_N50 3.1e-15 (the case the kernel's refinement round is for)."""
    lin, P, r, _, dP, s = linear_p_case(name)
    tol = 64.0 * sp.e_ref_p()
    B = P.shape[0]
    assert np.all(s["flag"] == 0), s["flag"]
    assert s["dw"].shape == (B, lin.n_w_ms, lin.nx) and s["du0"].shape == (B, lin.nu, lin.nx)
    worst = 0.0
    for b in range(B):
        ref, ok = restated_p(lin, r, b, dP[b], LD)
        assert ok
        worst = max(worst, sr.rel_err(s["dw"][b], ref))
    print(f"{name}: worst error against the long-double restatement {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_x0_directions_reproduce_sens_x0(mpcx, name):
    """2. dP = [I; 0] against Solver.sens_x0 at the same point: 64 x (e_ref + e_ref_p) relative to
    max(1, |entry|) -- both results lie within their own bound of the same long-double recursion.
    Measured on one MI355X: the same bits in all four cases (both end with a refinement step on the
    same system; tolerance 1.6e-13)."""
    lin, P, r, sx, solver = linear_case(name)
    B, nx = P.shape[0], lin.nx
    dP = np.zeros((B, nx, P.shape[1]))
    dP[:, np.arange(nx), np.arange(nx)] = 1.0
    s = solver.sens_p(P, r, dP)
    tol = 64.0 * (sr.e_ref() + sp.e_ref_p())
    assert np.all(s["flag"] == 0)
    worst = max(sr.rel_err(s["dw"][b], sx["dw_dx0"][b]) for b in range(B))
    print(f"{name}: worst difference to sens_x0 {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol
    assert bits(s["dw"][:, :nx]) == bits(np.broadcast_to(np.eye(nx), (B, nx, nx)))


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_active_set(mpcx, name):
    """3. Against the parametric active-set sensitivities (helper (c): active variables fixed, no barrier
    term, right-hand side (-r, dx0)).  Asserted on the inputs: every bounded variable is active (slack
    < 1e-6, |lam_x| > 1e-2) or has |lam_x| < 1e-7.  Tolerance: 8 x the distance helper (a) in long
    double, fed the same GPU point, has to (c), the rule of test_gpu_sens.py
    test_linear_against_the_active_set; the rows of the active variables are within it of zero.
    Measured distances of (a) to (c) on one MI355X, worst instance of each case: padded_dint_N8 2.2e-5
    (the instance without an active bound; 1.1e-7 to 1.6e-6 on the saturated ones), lin4x2_N12 5.6e-6,
    cartpole_qp_N50 5.2e-8, ltv_N40 2.9e-7; the GPU's distance to (c) equals (a)'s to four digits in
    every instance."""
    lin, P, r, _, dP, s = linear_p_case(name)
    lb, ub = sr.ocp_bounds(lin)
    for b in range(P.shape[0]):
        act, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, lin.nx)
        assert ok, (name, b, "a bounded variable is neither active nor without a multiplier")
        A, Bm, H = sr.linear_operands(lin, b)
        ref = sp.active_set_sens_p(A, Bm, H, act, *sp.linear_rhs(lin, dP[b], b))
        dist = float(np.max(np.abs(np.asarray(restated_p(lin, r, b, dP[b], LD)[0], np.float64) - ref)))
        err = float(np.max(np.abs(s["dw"][b] - ref)))
        print(f"{name} b={b}: {int(act.sum())} active, (a)-(c) {dist:.3e}, GPU-(c) {err:.3e}")
        assert err <= 8.0 * dist
        if act.any():
            assert np.max(np.abs(s["dw"][b][act])) <= 8.0 * dist


# ------------------------------------------------------------------------------------------
# 4. nonlinear models against central differences of the solver itself along the directions
# ------------------------------------------------------------------------------------------
NONLINEAR_CASES = ("unicycle_N10", "unicycle_N30", "unicycle_bounded_N10", "unicycle_tracking_N10", "kin_bicycle_N10",
                   "cartpole_N20", "dyn_bicycle_N10")


def nonlinear_p_problem(name):
    """(ocp, P, ipopt options): test_gpu_sens.py's cases and draws, and the unicycle tracking problem
    (node cost, stage references) on the circular reference.  Its input references are the circle's own
    (v, omega) = (0.1, 0.1): circular_reference keeps the script's (1, 1), and v_ref = 1 is the bound
    |v| <= 1 itself, so the last input (which no later cost sees) sits weakly on it in every instance
    and no solution is strictly complementary.  The draws picked from the pool of 24 are strictly
    complementary ones with 2 to 4 active input bounds each.  Solved to tol = 1e-10: the row of an
    active input with multiplier z moves by mu / z^2 with the barrier parameter mu at which a solve
    happens to stop, and the nominal and the perturbed solves need not stop at the same one -- 1e-5 for
    z ~ 1e-2 at the default tolerance's mu ~ 1e-9, above the yardstick of this quickly converging
    problem (FD spread 9e-7 at the default tolerance; |GPU - FD| was 7.3e-6 there)."""
    if name != "unicycle_tracking_N10":
        return nonlinear_problem(name)
    import mpcx
    from mpcx import ocp as ocp_mod

    B, N, pick = 24, 10, [2, 4, 5, 17]
    rng = np.random.default_rng(8)
    ocp = mpcx.unicycle_tracking(N=N)
    ref = ocp_mod.circular_reference(rng.uniform(0, 20 * math.pi, B), 0, N)
    ref[..., 3:] = 0.1
    x0 = ref[:, 0, :3] + rng.normal(0, 0.3, (B, 3))
    P = np.concatenate([x0, ref.reshape(B, -1)], axis=1)[pick]
    return ocp, np.ascontiguousarray(P), {"max_iter": 500, "tol": 1e-10}


def nonlinear_directions(ocp, P, name):
    """x0_xref: the nx unit directions of x_ref; stage references: two seeded directions of unit max-norm
    over the reference part, the x0 part zero"""
    B, n_p, nx = P.shape[0], P.shape[1], ocp.nx
    if ocp.param == "x0_xref":
        dP = np.zeros((B, nx, n_p))
        dP[:, np.arange(nx), nx + np.arange(nx)] = 1.0
        return dP
    rng = np.random.default_rng(200 + NONLINEAR_CASES.index(name))
    dP = np.zeros((B, 2, n_p))
    dP[:, :, nx:] = rng.uniform(-1.0, 1.0, (B, 2, n_p - nx))
    return dP / np.max(np.abs(dP), axis=2, keepdims=True)


@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_nonlinear_against_finite_differences(mpcx, name):
    """4. dw = (dw*/dP) dP against central differences of solve_batch along P +- h dP, warm-started from
    the nominal solution, at h = 1e-3 and h = 1e-4.  Yardstick: the spread between the two estimates
    (their largest difference over the instance's entries); tolerance 4 x spread + 1e-6 against their
    mean -- test 3 of test_gpu_sens.py.  An instance whose active-set class (helpers/sens_ref.py
    classify) changes between the two sides is left out, at most one per case; the nominal solutions
    are strictly complementary (asserted).  The draws are test_gpu_sens.py's, which hold under these
    perturbations too: one instance is left out in unicycle_N10 and in unicycle_N30, none elsewhere.
    Measured on one MI355X, worst instance of each case (FD spread, |GPU - FD|): unicycle_N10 2.2e-5,
    8.0e-6; unicycle_N30 1.9e-4, 1.4e-4; unicycle_bounded_N10 2.3e-5, 3.6e-5; unicycle_tracking_N10
    2.3e-6, 1.2e-6; kin_bicycle_N10 5.8e-6, 2.5e-6; cartpole_N20 1.4e-6, 6.9e-7 (entries up to 81);
    dyn_bicycle_N10 1.4e-4, 7.0e-5."""
    ocp, P, opts = nonlinear_p_problem(name)
    solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": opts})
    nx, B = ocp.nx, P.shape[0]
    lb, ub = sr.ocp_bounds(ocp)
    nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), nom["status"]
    dP = nonlinear_directions(ocp, P, name)
    m = dP.shape[1]
    s = solver.sens_p(P, nom, dP)
    assert np.all(s["flag"] == 0), s["flag"]
    assert s["dw"].shape == (B, nom["w"].shape[1], m)
    act0 = []
    for b in range(B):
        a, ok = sr.classify(nom["w"][b], nom["lam_x"][b], lb, ub, nx)
        assert ok, (name, b, "the nominal solution is not strictly complementary")
        act0.append(a)
    same = np.ones(B, bool)
    fd = {}
    for h in (1e-3, 1e-4):
        d = np.zeros((B, nom["w"].shape[1], m))
        for j in range(m):
            side = []
            for sgn in (1.0, -1.0):
                r = solver.solve_batch(P + sgn * h * dP[:, j], w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"])
                for b in range(B):
                    a, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, nx)
                    same[b] &= bool(r["status"][b] <= 1 and ok and np.array_equal(a, act0[b]))
                side.append(r["w"])
            d[:, :, j] = (side[0] - side[1]) / (2 * h)
        fd[h] = d
    assert np.count_nonzero(~same) <= 1, (name, "instances whose active set changes", np.flatnonzero(~same))
    for b in np.flatnonzero(same):
        spread = float(np.max(np.abs(fd[1e-3][b] - fd[1e-4][b])))
        err = float(np.max(np.abs(s["dw"][b] - 0.5 * (fd[1e-3][b] + fd[1e-4][b]))))
        print(f"{name} b={b}: {int(act0[b].sum())} active, FD spread {spread:.3e}, |GPU - FD| {err:.3e}, "
              f"|dw| {np.max(np.abs(s['dw'][b])):.3f}")
        assert err <= 4.0 * spread + 1e-6, (name, b)
        assert np.max(np.abs(s["dw"][b])) > 1e-3  # the solution does move with the references


# ------------------------------------------------------------------------------------------
# 5. exact properties
# ------------------------------------------------------------------------------------------
def test_exact_properties_unicycle(mpcx):
    """The X_0 rows of dw are dP[:, :, :nx] bit for bit; a zero direction gives zeros; column j of an
    m-column launch (and of a call split over several launches) has the bits of a one-column launch;
    instance b inside B = 5 has the bits of the same instance alone; sens_xref has the bits of sens_p
    with identity directions on x_ref; du0 is rows nx..nx+nu of dw; the single-shooting form returns
    the control rows."""
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("exact_p", "mi355x", ocp, {"ipopt": REF_OPTS})
    P = unicycle_P(5, 1)
    r = solver.solve_batch(P)
    dP = np.random.default_rng(9).normal(size=(5, 5, 6))  # five directions: launches of 3 and 2 columns
    s = solver.sens_p(P, r, dP)
    assert np.all(s["flag"] == 0) and s["dw"].shape == (5, 53, 5)
    assert bits(s["dw"][:, :3]) == bits(np.swapaxes(dP[:, :, :3], 1, 2))
    assert bits(s["du0"]) == bits(s["dw"][:, 3:5])
    s3 = solver.sens_p(P, r, dP[:, :3])
    assert bits(s3["dw"]) == bits(s["dw"][:, :, :3])
    for j in range(5):
        one = solver.sens_p(P, r, dP[:, j])  # (B, n_p): a single direction
        assert one["dw"].shape == (5, 53, 1) and bits(one["dw"][:, :, 0]) == bits(s["dw"][:, :, j]), j
    zero = solver.sens_p(P, r, np.zeros((5, 2, 6)))
    assert np.all(zero["flag"] == 0) and not zero["dw"].any() and not zero["du0"].any()
    for b in range(5):
        solo = solver.sens_p(P[b:b + 1], {k: r[k][b:b + 1] for k in ("w", "lam_g", "lam_x")}, dP[b:b + 1, :3])
        assert bits(solo["dw"][0]) == bits(s3["dw"][b]) and solo["flag"][0] == 0, b
    eye = np.zeros((5, 3, 6))
    eye[:, np.arange(3), 3 + np.arange(3)] = 1.0
    sx, se = solver.sens_xref(P, r), solver.sens_p(P, r, eye)
    assert bits(sx["dw_dxref"]) == bits(se["dw"]) and bits(sx["Kr"]) == bits(se["du0"]) and bits(sx["flag"]) == bits(se["flag"])
    assert not sx["dw_dxref"][:, :3].any() and np.max(np.abs(sx["Kr"])) > 1e-3
    ss = mpcx.nlpsol("ss_p", "mi355x", mpcx.unicycle_point_to_point(N=10, formulation="single_shooting"),
                     {"ipopt": REF_OPTS})
    su = ss.sens_p(P, r, dP[:, :3])
    rows = np.concatenate([3 + 5 * k + np.arange(2) for k in range(10)])
    assert su["dw"].shape == (5, 20, 3) and bits(su["dw"]) == bits(s3["dw"][:, rows]) and bits(su["du0"]) == bits(s3["du0"])
    with pytest.raises(ValueError):
        solver.sens_p(P, r, np.zeros((4, 3, 6)))


@pytest.mark.parametrize("name", ["padded_dint_N8", "ltv_N40"])
def test_exact_rows_linear(mpcx, name):
    lin, P, r, solver, dP, s = linear_p_case(name)
    assert bits(s["dw"][:, :lin.nx]) == bits(np.swapaxes(dP[:, :, :lin.nx], 1, 2))
    assert bits(s["du0"]) == bits(s["dw"][:, lin.nx:lin.nx + lin.nu])
    one = solver.sens_p(P, r, dP[:, 1])
    assert bits(one["dw"][:, :, 0]) == bits(s["dw"][:, :, 1])
    with pytest.raises(ValueError):  # stage references: there is no single target
        solver.sens_xref(P, r)


# ------------------------------------------------------------------------------------------
# 6. host and device entry points agree
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unicycle_N10", "padded_dint_N8"])
def test_device_loop_equals_host_call(mpcx, name):
    """DeviceLoop.sens_p after solve() and after step() (P already advanced: not a solution's own x0,
    but the same data) against Solver.sens_p on the loop's tensors copied back, bit for bit."""
    import torch
    from mpcx.device import DeviceLoop

    if name == "unicycle_N10":
        ocp, P = mpcx.unicycle_point_to_point(N=10), unicycle_P(5, 1)
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": REF_OPTS})
    else:
        ocp, P = linear_problem(name)
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": {"max_iter": 300}})
    pd = solver._pad
    B, m = P.shape[0], ocp.nx
    dP = np.random.default_rng(10).normal(size=(B, m, P.shape[1]))
    dPk = dP if pd is None else pd.scatter(dP.reshape(B * m, -1), pd.p_idx, pd.n_p_pad).reshape(B, m, -1)
    loop = DeviceLoop(solver, P, device="cuda:0")
    d_dP = torch.from_numpy(np.ascontiguousarray(dPk)).to("cuda:0")
    for phase in ("solve", "step"):
        getattr(loop, phase)()
        dw, flag = loop.sens_p(d_dP)
        torch.cuda.synchronize()
        host = {k: t.cpu().numpy() for k, t in (("P", loop.P), ("w", loop.w), ("lam_g", loop.lam), ("lam_x", loop.lamx))}
        dw = dw.cpu().numpy()
        if pd is not None:  # the loop's tensors hold the kernel's padded layout
            host = {"P": host["P"][:, pd.p_idx], "w": host["w"][:, pd.w_idx], "lam_g": host["lam_g"][:, pd.g_idx],
                    "lam_x": host["lam_x"][:, pd.w_idx]}
            dw = dw[:, pd.w_idx]
        s = solver.sens_p(host["P"], host, dP)
        assert np.all(s["flag"] == 0) and bits(flag.cpu().numpy()) == bits(s["flag"]), phase
        assert bits(dw) == bits(s["dw"]), phase
    out = torch.full((B, solver._h.n_w, m), 7.0, dtype=torch.float64, device="cuda:0")
    got = loop.sens_p(d_dP, dw_out=out)[0]
    torch.cuda.synchronize()
    assert got is out and not bool((out == 7.0).any())
    with pytest.raises(ValueError):
        loop.sens_p(d_dP, dw_out=out[:, :, :1])
    with pytest.raises(ValueError):
        loop.sens_p(torch.zeros((B, loop._knx + 1, loop.P.shape[1]), dtype=torch.float64, device="cuda:0"))


# ------------------------------------------------------------------------------------------
# 7. irregular instances: ordinary statuses, nothing faults; refusals
# ------------------------------------------------------------------------------------------
def assert_only_irregular(s, bad, regular=None):
    for b in range(s["flag"].shape[0]):
        if b == bad:
            assert s["flag"][b] == 1
            assert np.all(np.isnan(s["dw"][b])) and np.all(np.isnan(s["du0"][b]))
        else:
            assert s["flag"][b] == 0
            assert np.all(np.isfinite(s["dw"][b]))
            if regular is not None:  # the neighbours keep their bits
                assert bits(s["dw"][b]) == bits(regular["dw"][b]), b


def test_variable_on_its_bound_is_flagged(mpcx):
    lin, P, r, solver, dP, s = linear_p_case("padded_dint_N8")
    w = r["w"].copy()
    w[2, lin.nx + (lin.nx + lin.nu) * 3] = 1.0  # U_3 of instance 2 placed on its upper bound
    assert_only_irregular(solver.sens_p(P, {"w": w, "lam_g": r["lam_g"], "lam_x": r["lam_x"]}, dP), 2, s)


def test_indefinite_stage_is_flagged(mpcx):
    """A negative input weight on the last stage of instance 1 of 3 (test_gpu_sens.py's case)."""
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
    solver = mpcx.nlpsol("indef_p", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    P = lin.params(rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    point = {"w": np.zeros((B, lin.n_w_ms)), "lam_g": np.zeros((B, lin.n_g_ms)), "lam_x": np.zeros((B, lin.n_w_ms))}
    assert_only_irregular(solver.sens_p(P, point, rng.normal(size=(B, 2, P.shape[1]))), 1)


def test_refusals(mpcx):
    """MPCX_EINVAL with a message and nothing launched, on both entry points: m = 0 and m = nx + 1, a
    null dP or dw, N = 64, the path-frame bicycle (and B < 1, a null point)."""
    import torch
    from mpcx import _lib, ode

    lib = _lib.load()
    EINVAL = -1

    def host_call(solver, B=2, m=1, n_null=()):
        h = solver._h
        n, mm = max(B, 1), max(m, 1)
        arr = [np.zeros((n, h.n_p)), np.zeros((n, h.n_w)), np.zeros((n, h.n_g)), np.zeros((n, h.n_w)),
               np.zeros((n, mm, h.n_p)), np.full((n, h.n_w, mm), 7.0)]
        a = [None if i in n_null else _lib.dptr(v) for i, v in enumerate(arr)]
        rc = lib.mpcx_sens_p(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], m, a[5], None)
        assert rc != 0 and np.all(arr[5] == 7.0)
        return rc, lib.mpcx_last_error().decode()

    solver = mpcx.nlpsol("ok_p", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    long = mpcx.nlpsol("n64_p", "mi355x", mpcx.unicycle_point_to_point(N=64), {"ipopt": REF_OPTS})
    path = mpcx.nlpsol("path_p", "mi355x", ode.path_bicycle_lane_keeping(N=20), {"ipopt": {"max_iter": 100}})
    buf = torch.zeros(2 * long._h.n_w * 4, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())

    def dev_call(h, B=2, m=1, lam_g=p, dP=p, dw=p):
        rc = lib.mpcx_sens_p_dev(h.ptr, B, p, p, lam_g, p, dP, m, dw, None, None)
        return rc, lib.mpcx_last_error().decode()

    for call, hs in ((host_call, (solver, long, path)), (dev_call, (solver._h, long._h, path._h))):
        ok, n64, pth = hs
        for m in (0, 4):
            rc, msg = call(ok, m=m)
            assert rc == EINVAL and "between 1 and nx" in msg, (m, msg)
        for B in (0, -3):
            rc, msg = call(ok, B=B)
            assert rc == EINVAL and "B must be >= 1" in msg
        rc, msg = call(n64)
        assert rc == EINVAL and "N >= 64" in msg
        rc, msg = call(pth)
        assert rc == EINVAL and "path-frame bicycle" in msg
    for i in range(6):  # P, w, lam_g, lam_x, dP, dw
        rc, msg = host_call(solver, n_null=(i,))
        assert rc == EINVAL and "required" in msg
    for kw in ({"lam_g": None}, {"dP": None}, {"dw": None}):
        rc, msg = dev_call(solver._h, **kw)
        assert rc == EINVAL and "required" in msg
    rc = lib.mpcx_sens_p_dev(None, 2, p, p, p, p, p, 1, p, None, None)
    assert rc == EINVAL and "null handle" in lib.mpcx_last_error().decode()
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched
