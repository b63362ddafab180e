"""GPU tests of the seven sensitivity calls (csrc/sens.h: sens_x0, sens_p, sens_vjp, sens_bounds and its VJP,
sens_weights and its VJP) on the NONLINEAR models against an exact long-double reference.

Reference: tests/helpers/sens_nonlinear_ref.py -- the hyper-dual stage derivatives of helpers/stage_derivs_ref.py in
np.longdouble (A_k, B_k, H_k = hess(q_k + lam_{k+1}^T F_k), no truncation) fed to the long-double restatements of the
kernels' two rounds, at the GPU's own solve_batch result.  tests/test_sens_nonlinear_cpu.py checks that reference by
itself.  Every instance and every entry is compared, relative to max(1, |entry|) (sens_ref.rel_err).

Bound per case and call: 64 x max(E64(case, call), the helper's linear yardstick e_ref*()), where E64 is the same
pipeline run in float64 against its long-double run AT THE SAME POINT -- computed here from the reference alone,
never from the kernel.  64 is the factor of every linear sensitivity test (the kernel's other operation order --
scan against chain, fma contraction -- and its own float64 derivative evaluation, which tests/test_gpu_stage_derivs.py
holds to 16 x E64 per block).  Conditions, asserted, not measured: every solve status <= 1, every flag 0, the
reference's factors regular on every instance, E64 <= 1e-12.

Directions and cotangents: m = nx per call, seeded normal over the whole row (every column slot is used); the
weights' relative to each weight, as tests/test_sens_nonlinear_cpu.py explains.

Measured on one MI355X: error / bound, the worst instance of each case (each test prints error and E64 too).  The
errors themselves are 2.4e-17 to 5.2e-15 (1.2e-14 on the bounds call of unicycle_bounded_N15), the cart-pole's up to
1.3e-13 (its E64 is that much larger: up to 2.0e-13); the worst share of a bound is 0.051.  "-": the call is not made
on that case; 0: below 5e-4 (the bounds pair where no bound is active: an O(mu) result, errors 1e-21 and less).
                                x0     p      vjp    bounds b_vjp  weights w_vjp
  own    unicycle_N10           0.009  0.017  0.003  0.002  0.001  0.001  0.003
  own    unicycle_bounded_N10   0.009  0.010  0.005  0.002  0.002  0.001  0.003
  own    unicycle_N30           0.020  0.016  0.014  0.002  0.002  0.001  0.020
  own    kin_bicycle_N10        0.009  0.004  0.004  0      0      0      0.001
  own    cartpole_N20           0.013  0.015  0.023  0      0      0.051  0.012
  own    path_bicycle_N20       0.017  -      -      0      0      0      0.021
  own    dyn_bicycle_N10        0.019  0.004  0.004  0      0      0      0.001
  own    unicycle_tracking_N10  -      0.005  0.005  -      -      0.001  0.003
  drawn  kin_bicycle_N10        0.016  0.005  0.009  0.001  0.001  0      0.002   (48 variables with Sigma > 1, up to 9e8)
  drawn  cartpole_N20           0.014  0.016  0.026  0.001  0.001  0.017  0.025   (8, up to 4e5)
  drawn  path_bicycle_N20       0.012  -      -      0.001  0.001  0      0.015   (16, up to 1e7)
  drawn  dyn_bicycle_N10        0.008  0.006  0.004  0.002  0.004  0      0.001   (13, up to 2e11)
  edge   unicycle_N15           0.011  0.013  0.007  0.003  0.002  0.001  0.010
  edge   unicycle_N31           0.016  0.011  0.006  0.003  0.003  0.001  0.006
  edge   unicycle_N63           0.013  0.009  0.005  0.002  0.002  0.001  0.015
  edge   kin_bicycle_N15        0.015  0.018  0.018  0.004  0.001  0.002  0.006
  edge   dyn_bicycle_N15        0.022  0.008  0.006  0      0      0      0.002
  edge   cartpole_N31           0.014  0.021  0.007  0      0      0.022  0.011
  edge   path_bicycle_N31       0.011  -      -      0      0      0.001  0.009
  edge   unicycle_bounded_N15   0.024  0.019  0.004  0.050  0.016  0.002  0.017   (Sigma_x on node N up to 1.9e8)
sens_p with dP = [I; 0] gave sens_x0's bits in every case (asserted only within the sum of the two bounds).
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sens_nonlinear_ref as sn  # noqa: E402
import sens_ref as sr  # noqa: E402
from test_gpu_sens import NONLINEAR_CASES, nonlinear_problem, unicycle_P  # noqa: E402
from test_gpu_sens_bounds import drawn_in_bounds  # noqa: E402
from test_gpu_sens_p import nonlinear_p_problem  # noqa: E402
from test_sens_nonlinear_cpu import calls_of, directions  # noqa: E402

LD = np.longdouble
ODE_CASES = ("kin_bicycle_N10", "cartpole_N20", "path_bicycle_N20", "dyn_bicycle_N10")
EDGE_CASES = ("unicycle_N15", "unicycle_N31", "unicycle_N63", "kin_bicycle_N15", "dyn_bicycle_N15", "cartpole_N31",
              "path_bicycle_N31", "unicycle_bounded_N15")


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def edge_problem(name):
    """(ocp, P, ipopt options) of an edge shape: N + 1 a power of two, so that node N sits on the last lane of its
    group, and B = 5, so that the last wave has surplus lanes (G = 16: 4 + 1 groups).  Starts drawn as
    test_gpu_sens.nonlinear_problem draws them, from seeds of their own."""
    import dataclasses
    import math

    import mpcx
    from mpcx import ode

    model, N = name.rsplit("_N", 1)
    N, B = int(N), 5
    if model in ("unicycle", "unicycle_bounded"):
        ocp, opts = mpcx.unicycle_point_to_point(N=N), nonlinear_problem("unicycle_N10")[2]
        if model == "unicycle_bounded":  # y <= 1 as unicycle_bounded_N10: a state bound on node N, the group's last lane
            ocp = dataclasses.replace(ocp, x_ub=(math.inf, 1.0, math.inf))
        return ocp, unicycle_P(24, 21)[[0, 1, 2, 3, 4]], opts
    if model == "kin_bicycle":
        rng = np.random.default_rng(22)
        ocp = ode.kinematic_bicycle_tracking(N=N)
        ref = ode.bicycle_circular_reference(rng.uniform(0, 20 * math.pi, B), 0, N)
        return ocp, ocp.params(ref[:, 0, :3] + rng.normal(0, 0.1, (B, 3)), ref), {"max_iter": 500}
    if model == "cartpole":
        rng = np.random.default_rng(23)
        ocp = ode.cartpole_swingup(N=N)
        x0 = rng.uniform(-1, 1, (B, 4)) * np.array([0.5, 0.3, 0.3, 0.3])
        xr = np.zeros((B, 4))
        xr[:, 0] = rng.uniform(-1, 1, B)
        return ocp, ocp.params(x0, xr), {"max_iter": 1000}
    if model == "dyn_bicycle":
        rng = np.random.default_rng(24)
        ocp = ode.dynamic_bicycle_lane_change(N=N)
        ref = np.zeros((B, N, 8))
        ref[..., 0] = 6.0 * ocp.T * np.arange(N)
        ref[..., 3] = 6.0
        x0 = ref[:, 0, :6] + rng.normal(0, 1, (B, 6)) * np.array([0.2, 0.2, 0.05, 0.3, 0.1, 0.05])
        return ocp, ocp.params(x0, ref), {"max_iter": 1000}
    assert model == "path_bicycle"
    rng = np.random.default_rng(26)
    ocp = ode.path_bicycle_lane_keeping(N=N)
    rows = np.zeros((B, N, 6))
    rows[..., 0] = rng.uniform(-0.5, 0.5, (B, 1))
    rows[..., 2] = rng.uniform(5.0, 10.0, (B, 1))
    x = np.stack([rows[:, 0, 0] + rng.uniform(-0.3, 0.3, B), rng.normal(0, 0.02, B), rows[:, 0, 2] + rng.normal(0, 0.3, B)],
                 axis=1)
    return ocp, ode.path_bicycle_params(ocp, x, 0.0, rows), {"max_iter": 1000, "tol": 1e-8}


@functools.lru_cache(maxsize=None)
def gpu_case(kind, name):
    """(ocp, P, solver, solve result, lb, ub (B, n_w), per-instance bounds?, the reference's points in long double
    and in float64) of a case, solved once on the GPU and shared; never modified.
    kind "own": the case under the problem's own bounds; "drawn": under test_gpu_sens_bounds.drawn_in_bounds at
    tol = 1e-10; "edge": edge_problem."""
    import mpcx

    ocp, P, opts = edge_problem(name) if kind == "edge" else nonlinear_p_problem(name)
    B = P.shape[0]
    lb0, ub0 = sr.ocp_bounds(ocp)
    lb, ub = np.tile(lb0, (B, 1)), np.tile(ub0, (B, 1))
    if kind == "drawn":
        solver = mpcx.nlpsol(name + "_nl_drawn", "mi355x", ocp, {"ipopt": dict(opts, tol=1e-10)})
        free = solver.solve_batch(P)
        assert np.all(free["status"] <= 1), free["status"]
        lb, ub = drawn_in_bounds(ocp, free["w"])
        nom = solver.solve_batch(P, lbw=lb, ubw=ub)
    else:
        solver = mpcx.nlpsol(name + "_nl_" + kind, "mi355x", ocp, {"ipopt": opts})
        nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), (kind, name, nom["status"])
    for v in nom.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    pts = list(zip(sn.points(ocp, P, nom, lb, ub, LD), sn.points(ocp, P, nom, lb, ub, np.float64)))
    return ocp, P, solver, nom, lb, ub, kind == "drawn", pts


def device_call(solver, call, P, nom, args, lb, ub, per_instance):
    """(the call's outputs of every instance stacked as sens_nonlinear_ref.stacked stacks the reference's, flags):
    args[b] = the directions of instance b.  sens_x0 / sens_p / sens_vjp take bounds shared by a batch only: with
    per-instance bounds they are called instance by instance (an instance's bits do not depend on its batch)."""
    B = P.shape[0]
    stack = lambda i: np.stack([a[i] for a in args])  # noqa: E731
    if call in ("x0", "p", "vjp"):
        def one(rows, kw):
            pt = {k: nom[k][rows] for k in ("w", "lam_g", "lam_x")}
            if call == "x0":
                s = solver.sens_x0(P[rows], pt, **kw)
                return [s["dw_dx0"]], s["flag"]
            if call == "p":
                s = solver.sens_p(P[rows], pt, stack(0)[rows], **kw)
                return [s["dw"]], s["flag"]
            s = solver.sens_vjp(P[rows], pt, stack(0)[rows], **kw)
            return [s["gP"]], s["flag"]

        if per_instance:
            parts = [one(slice(b, b + 1), {"lbw": lb[b], "ubw": ub[b]}) for b in range(B)]
            outs, flag = [np.concatenate([p[0][0] for p in parts])], np.concatenate([p[1] for p in parts])
        else:
            outs, flag = one(slice(None), {})
    else:
        kw = {"lbw": lb, "ubw": ub} if per_instance else {}
        if call == "bounds":
            s = solver.sens_bounds(P, nom, stack(0), stack(1), **kw)
            outs = [s["dw"]]
        elif call == "bounds_vjp":
            s = solver.sens_bounds_vjp(P, nom, stack(0), **kw)
            outs = [s["glbw"], s["gubw"]]
        elif call == "weights":
            s = solver.sens_weights(P, nom, dQ=stack(0), dR=stack(1), **kw)
            outs = [s["dw"]]
        else:
            s = solver.sens_weights_vjp(P, nom, stack(0), **kw)
            outs = [s["gQk"], s["gRk"], s["gQ"], s["gR"]]
        flag = s["flag"]
    return [np.concatenate([np.ravel(o[b]) for o in outs]) for b in range(B)], flag


def check(kind, name, calls=None):
    """Every call of the case against its reference; returns {call: (error, bound, E64)} after asserting the
    conditions and the bounds (all calls are measured and printed before the first assertion on a bound)."""
    ocp, P, solver, nom, lb, ub, per_instance, pts = gpu_case(kind, name)
    B, out = P.shape[0], {}
    for call in calls_of(ocp) if calls is None else calls:
        args = [directions(call, ocp, P.shape[1], 300 + b) for b in range(B)]
        got, flag = device_call(solver, call, P, nom, args, lb, ub, per_instance)
        assert np.all(flag == 0), (kind, name, call, flag)
        E = err = 0.0
        for b, (pt, pt64) in enumerate(pts):
            sol = {k: nom[k][b] for k in ("w", "lam_g", "lam_x")}
            e, ref, ok = sn.e64(call, ocp, P[b], sol, lb[b], ub[b], args[b], pt, pt64)
            assert ok, (kind, name, call, b, "the reference's factors are not regular")
            assert got[b].shape == ref.shape and np.all(np.isfinite(got[b]))
            E, err = max(E, e), max(err, sr.rel_err(got[b], ref))
        out[call] = (err, 64.0 * max(E, sn.linear_yardstick(call)), E)
    n_act = sum(int(np.sum(np.asarray(pt.Sig, np.float64) > 1.0)) for pt, _ in pts)
    print(f"\n{kind} {name} (B = {B}, {n_act} variables with Sigma > 1, Sigma up to "
          f"{max(float(np.max(pt.Sig)) for pt, _ in pts):.1e}):  "
          + "  ".join(f"{c} {e / bd:.3f} (err {e:.1e}, E64 {E:.1e})" for c, (e, bd, E) in out.items()))
    for c, (e, bd, E) in out.items():
        assert E <= 1e-12, (kind, name, c, "E64", E)
    for c, (e, bd, E) in out.items():
        assert e <= bd, (kind, name, c, e, bd)
    return out


@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_own_bounds_against_the_reference(mpcx, name):
    """The seven cases of tests/test_gpu_sens.py at the GPU's own solutions, all seven calls (sens_p / sens_vjp skip
    the path-frame bicycle, which refuses them)."""
    check("own", name)


def test_tracking_unicycle_against_the_reference(mpcx):
    """The node-cost unicycle with stage references (tests/test_gpu_sens_p.py, tests/test_gpu_sens_weights.py):
    sens_p / sens_vjp over the whole row of stage references, and the weights pair."""
    check("own", "unicycle_tracking_N10", ("p", "vjp", "weights", "weights_vjp"))


@pytest.mark.parametrize("name", ODE_CASES)
def test_drawn_in_bounds_against_the_reference(mpcx, name):
    """The four ODE models under per-instance (B, n_w) bounds drawn in to 0.8 of each instance's largest free move of
    every input (test_gpu_sens_bounds.drawn_in_bounds, tol = 1e-10): active and weakly active bounds, where central
    differences are no reference.  The bounds are felt: some Sigma > 1 (asserted)."""
    check("drawn", name)
    pts = gpu_case("drawn", name)[7]
    assert max(float(np.max(pt.Sig)) for pt, _ in pts) > 1.0


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_shapes_against_the_reference(mpcx, name):
    """N + 1 = 16, 32, 64: node N on the last lane of its group; B = 5: surplus lanes in the last wave.  One case
    beyond the bare models: unicycle_bounded_N15, whose state bound y <= 1 is active on node N itself (asserted:
    Sigma > 1 there in some instance; 2.9e6 to 1.9e8 in three of the five), so that the last lane carries a Sigma_x."""
    check("edge", name)
    if name == "unicycle_bounded_N15":
        ocp, pts = gpu_case("edge", name)[0], gpu_case("edge", name)[7]
        assert max(float(np.max(pt.Sig[ocp.N, :ocp.nx])) for pt, _ in pts) > 1.0


@pytest.mark.parametrize("kind,name", [("own", n) for n in NONLINEAR_CASES] + [("edge", n) for n in EDGE_CASES])
def test_exact_checks_at_the_same_points(mpcx, kind, name):
    """K0 equals rows nx : nx + nu of dw_dx0 bit for bit; the X_0 rows of dw_dx0 are the identity; and sens_p with
    dP = [I; 0] equals sens_x0 within the sum of the two calls' bounds (the E64 of each at this case's points, from
    the reference alone; not for the path-frame bicycle, which sens_p refuses)."""
    ocp, P, solver, nom, lb, ub, _, pts = gpu_case(kind, name)
    nx, nu, B = ocp.nx, ocp.nu, P.shape[0]
    s = solver.sens_x0(P, nom)
    assert np.all(s["flag"] == 0)
    for b in range(B):
        assert bits(s["K0"][b]) == bits(s["dw_dx0"][b, nx:nx + nu])
        assert bits(s["dw_dx0"][b, :nx]) == bits(np.eye(nx))
    if "p" not in calls_of(ocp):
        return
    dP = np.zeros((B, nx, P.shape[1]))
    dP[:, np.arange(nx), np.arange(nx)] = 1.0
    sp_ = solver.sens_p(P, nom, dP)
    assert np.all(sp_["flag"] == 0)
    E = {"x0": 0.0, "p": 0.0}
    for b, (pt, pt64) in enumerate(pts):
        sol = {k: nom[k][b] for k in ("w", "lam_g", "lam_x")}
        E["x0"] = max(E["x0"], sn.e64("x0", ocp, P[b], sol, lb[b], ub[b], (), pt, pt64)[0])
        E["p"] = max(E["p"], sn.e64("p", ocp, P[b], sol, lb[b], ub[b], (dP[b],), pt, pt64)[0])
    bound = sum(64.0 * max(E[c], sn.linear_yardstick(c)) for c in E)
    err = sr.rel_err(sp_["dw"], s["dw_dx0"])
    print(f"\n{kind} {name}: sens_p([I; 0]) against sens_x0 {err:.3e} (bound {bound:.3e})")
    assert err <= bound
